"""The population and softmax calls against the oracle on the directed boards, on CPU (harness backend): the per-env
bodies the kernels run, at every kernel variant (tests/policy_directed_cases.py)."""
import pytest

import parity_cases as par
import policy_directed_cases as pd

DEV = "cpu"


def test_geometry_lists_cover_every_variant():
    """PICK_GEOMETRIES is the afterstate family's whole list; PLAY_GEOMETRIES keeps a geometry of every variant, every
    width and the four boards named in its comment, so that neither can shrink unnoticed."""
    assert pd.PICK_GEOMETRIES == par.AFTER_GEOMETRIES and len(pd.PICK_GEOMETRIES) == 24
    variants = {v for v, _ in par.AFTER_GEOMETRY_VARIANTS}
    assert len(variants) == 5
    assert {par.after_geometry_variant(C, R) for C, R in pd.PICK_GEOMETRIES} == variants
    assert {par.after_geometry_variant(C, R) for C, R in pd.PLAY_GEOMETRIES} == variants
    assert {C for C, _ in pd.PLAY_GEOMETRIES} == set(range(5, 13))
    assert set(pd.PLAY_MUST_HOLD) == {(6, 4), (9, 40), (10, 28), (12, 59)} <= set(pd.PLAY_GEOMETRIES)
    assert len(set(pd.PLAY_GEOMETRIES)) == len(pd.PLAY_GEOMETRIES)
    assert set(pd.PLAY_GEOMETRIES) <= set(par.AFTER_GEOMETRIES) | set(par.DIRECTED_GEOMETRIES)
    old_four = {(10, 20), (10, 40), (6, 10), (12, 20)}
    assert len(set(pd.PLAY_GEOMETRIES) - old_four) >= 13
    settings = set(pd.SOFTMAX_PLAY_SETTINGS)
    assert {(C, R) for C, R, T, d in settings if (T, d) == (1.0, False)} == set(pd.PLAY_GEOMETRIES)
    for C, R in ((10, 20), (10, 40)):
        assert (C, R, 20.0, False) in settings and (C, R, 1.0, True) in settings
    assert pd.K_PLAY == 6 and pd.MAX_DROPPED == 0.01
    assert (pd.MIN_OVER, pd.MIN_ENDED, pd.MIN_ALIVE, pd.MIN_CLEARED, pd.MIN_ONE_PLACEMENT) == (100, 200, 200, 300, 10)


@pytest.mark.parametrize("C,R", pd.PICK_GEOMETRIES)
def test_greedy_rows(host_backend, orc, C, R):
    pd.greedy_rows_directed(DEV, orc, C, R)


@pytest.mark.parametrize("C,R", pd.PICK_GEOMETRIES)
def test_softmax_rows(host_backend, orc, C, R):
    pd.softmax_rows_directed(DEV, orc, C, R)


@pytest.mark.parametrize("C,R", pd.PLAY_GEOMETRIES)
def test_play_linear(host_backend, orc, C, R):
    pd.play_linear_directed(DEV, orc, C, R)


@pytest.mark.parametrize("C,R,T,directed", pd.SOFTMAX_PLAY_SETTINGS)
def test_play_softmax(host_backend, orc, C, R, T, directed):
    pd.play_softmax_directed(DEV, orc, C, R, T, directed)


@pytest.mark.parametrize("C,R,T,directed", pd.SOFTMAX_PLAY_SETTINGS)
def test_play_softmax_equals_composition(host_backend, orc, C, R, T, directed):
    pd.play_softmax_composition_directed(DEV, orc, C, R, T, directed)
