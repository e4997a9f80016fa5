"""The two-piece lookahead on CPU (harness backend): the per-lane body the kernel runs, the sums, the pick and the host
logic of VecTetris.lookahead (tests/two_ply_cases.py has the cases)."""
import numpy as np
import pytest

import two_ply_cases as tp


@pytest.fixture(scope="module")
def lib():
    import harness_backend
    return harness_backend.binding()


@pytest.mark.parametrize("C,R,pieces", tp.TABLE_GEOMETRIES)
def test_table_vs_oracle(host_backend, orc, C, R, pieces):
    tp.table_vs_oracle("cpu", orc, C, R, pieces)


def test_sums_and_pick(host_backend):
    tp.sums_and_pick("cpu")


@pytest.mark.parametrize("C,R,pieces", [(10, 20, "default"), (10, 40, tp.gc.STANDARD7), (12, 59, "default")])
def test_position_independence(host_backend, C, R, pieces):
    tp.position_independence("cpu", C, R, pieces)


def test_many_workgroups(host_backend):
    tp.many_workgroups("cpu")


@pytest.mark.parametrize("form", tp.FOOTPRINT_FORMS)
@pytest.mark.parametrize("B", tp.fc.ROLLOUT_BATCHES)
@pytest.mark.parametrize("C,R", tp.fc.GEOMETRIES)
def test_footprint(lib, C, R, B, form):
    tp.footprint(lib, "cpu", C, R, B, form)


def test_plays(host_backend, golden_dir):
    """the stored trace is this run's (tests/golden/make_golden_two_ply.py writes it)"""
    np.testing.assert_array_equal(tp.plays("cpu"), tp.stored_trace(golden_dir))


def test_replay_mode(host_backend):
    tp.replay_mode("cpu")


def test_death_value_is_checked_by_the_library(host_backend):
    from tetris_amd import VecTetris, _lib
    env = VecTetris(10, 20, 3, device="cpu")
    for bad in (float("nan"), float("inf")):
        with pytest.raises(_lib.TetrisHipError):
            env.lookahead(death_value=bad)
    env.lookahead(death_value=0.0)
