"""The softmax linear policy on the MI355X: softmax_rows_kernel and play_softmax_kernel through the C-ABI and
VecTetris.sample_actions / play_sampled."""
import pytest

import population_cases as pc
import softmax_cases as sc

pytestmark = pytest.mark.gpu

FOOT_GEOMETRIES = [(10, 20), (10, 40), (6, 10), (12, 20)]


@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_logits_float64_and_draw(orc, C, R, pieces):
    """cases 1-3: logits bit-exact against NumPy float32; logz, logp and score against float64; the Gumbel draw"""
    sc.numerics("cuda", C, R, pieces, orc if (C, R) == (10, 20) else None)


def test_distribution():
    sc.distribution("cuda")


@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_limits(C, R, pieces):
    one, over = sc.limits("cuda", C, R, pieces)
    assert (C, R) != (6, 10) or (one > 0 and over > 0)


def test_reference_fixture():
    sc.reference_fixture("cuda")


@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_determinism_and_sharding(C, R, pieces):
    sc.determinism_and_sharding("cuda", C, R, pieces)


@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_play_equals_composition(C, R, pieces):
    played, frozen = sc.play_equals_composition("cuda", C, R, pieces)
    assert played > 0 and ((C, R) != (6, 10) or frozen > 0)


def test_play_equals_composition_negated():
    """games that end inside the launch"""
    played, frozen = sc.play_equals_composition("cuda", 10, 20, "default", K=40, w=-pc.BCTS, T=1.0)
    assert played > 0 and frozen > pc.B


def test_play_equals_composition_multi_workgroup():
    sc.play_equals_composition("cuda", 10, 20, "default", n=pc.B_MULTI, K=8)


def test_play_chunks_compose():
    sc.play_equals_composition("cuda", 10, 20, "default", K=24, split=[8, 16])


@pytest.mark.parametrize("n_steps", [1, 7])
@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_bad_rows(C, R, pieces, n_steps):
    sc.bad_rows("cuda", C, R, pieces, n_steps)


@pytest.mark.parametrize("null_arg", sc.SOFTMAX_ROWS_OPTIONAL)
@pytest.mark.parametrize("n", pc.FOOTPRINT_BATCHES)
@pytest.mark.parametrize("C,R", FOOT_GEOMETRIES)
def test_footprint_softmax_rows(C, R, n, null_arg):
    sc.footprint_softmax_rows("cuda", C, R, n, null_arg)


@pytest.mark.parametrize("null_arg", sc.PLAY_OPTIONAL)
@pytest.mark.parametrize("n", pc.FOOTPRINT_BATCHES)
@pytest.mark.parametrize("C,R", FOOT_GEOMETRIES)
def test_footprint_play(C, R, n, null_arg):
    sc.footprint_play("cuda", C, R, n, null_arg)


def test_facade():
    sc.facade("cuda")
