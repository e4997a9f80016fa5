"""The softmax linear policy on CPU (harness backend): the per-env bodies the kernels run (tet::softmax_pick_env,
tet::play_softmax_step_env), the C-ABI text and the host logic of sample_actions / play_sampled."""
import pytest

import population_cases as pc
import softmax_cases as sc

FOOT_GEOMETRIES = [(10, 20), (10, 40), (6, 10), (12, 20)]


@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_logits_float64_and_draw(host_backend, orc, C, R, pieces):
    """cases 1-3: logits bit-exact against NumPy float32; logz, logp and score against float64; the Gumbel draw"""
    sc.numerics("cpu", C, R, pieces, orc if (C, R) == (10, 20) else None)


def test_distribution(host_backend):
    sc.distribution("cpu")


@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_limits(host_backend, C, R, pieces):
    one, over = sc.limits("cpu", C, R, pieces)
    assert (C, R) != (6, 10) or (one > 0 and over > 0)


def test_reference_fixture(host_backend):
    sc.reference_fixture("cpu")


@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_determinism_and_sharding(host_backend, C, R, pieces):
    sc.determinism_and_sharding("cpu", C, R, pieces)


@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_play_equals_composition(host_backend, C, R, pieces):
    played, frozen = sc.play_equals_composition("cpu", C, R, pieces)
    assert played > 0 and ((C, R) != (6, 10) or frozen > 0)


def test_play_equals_composition_negated(host_backend):
    """games that end inside the launch"""
    played, frozen = sc.play_equals_composition("cpu", 10, 20, "default", K=40, w=-pc.BCTS, T=1.0)
    assert played > 0 and frozen > pc.B


def test_play_equals_composition_multi_workgroup(host_backend):
    sc.play_equals_composition("cpu", 10, 20, "default", n=pc.B_MULTI, K=8)


def test_play_chunks_compose(host_backend):
    sc.play_equals_composition("cpu", 10, 20, "default", K=24, split=[8, 16])


@pytest.mark.parametrize("n_steps", [1, 7])
@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_bad_rows(host_backend, C, R, pieces, n_steps):
    sc.bad_rows("cpu", C, R, pieces, n_steps)


@pytest.mark.parametrize("null_arg", sc.SOFTMAX_ROWS_OPTIONAL)
@pytest.mark.parametrize("n", pc.FOOTPRINT_BATCHES)
@pytest.mark.parametrize("C,R", FOOT_GEOMETRIES)
def test_footprint_softmax_rows(host_backend, C, R, n, null_arg):
    sc.footprint_softmax_rows("cpu", C, R, n, null_arg)


@pytest.mark.parametrize("null_arg", sc.PLAY_OPTIONAL)
@pytest.mark.parametrize("n", pc.FOOTPRINT_BATCHES)
@pytest.mark.parametrize("C,R", FOOT_GEOMETRIES)
def test_footprint_play(host_backend, C, R, n, null_arg):
    sc.footprint_play("cpu", C, R, n, null_arg)


def test_facade(host_backend):
    sc.facade("cpu")
