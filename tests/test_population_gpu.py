"""Greedy play of a population of linear policies on the MI355X: greedy_rows_kernel and play_linear_kernel through
the C-ABI and VecTetris.greedy_actions(rows=) / play."""
import pytest

import population_cases as pc

pytestmark = pytest.mark.gpu

FOOT_GEOMETRIES = [(10, 20), (10, 40), (6, 10), (12, 20)]


@pytest.mark.parametrize("rows_mode", ["rows", "null"])
@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_pick(orc, C, R, pieces, rows_mode):
    pc.pick("cuda", C, R, pieces, rows_mode, orc if (C, R) == (10, 20) else None)


@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_play_equals_step_many(C, R, pieces):
    played, frozen = pc.play_equals_step_many("cuda", C, R, pieces)
    assert played > 0 and ((C, R) != (6, 10) or frozen > 0)


def test_play_equals_step_many_negated():
    """games that end inside the launch: the frozen steps are the ones step_many counts as invalid"""
    played, frozen = pc.play_equals_step_many("cuda", 10, 20, "default", K=40, w=-pc.BCTS)
    assert played > 0 and frozen > pc.B


def test_play_equals_step_many_multi_workgroup():
    pc.play_equals_step_many("cuda", 10, 20, "default", n=pc.B_MULTI, K=8)


@pytest.mark.parametrize("C,R", sorted(pc.ORACLE_PLAY))
def test_play_vs_oracle(orc, C, R):
    pc.play_vs_oracle("cuda", orc, C, R, "default")


@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_chunks_compose(C, R, pieces):
    pc.chunks_compose("cuda", C, R, pieces)


def test_frozen_envs():
    pc.frozen_envs("cuda")


@pytest.mark.parametrize("n_steps", [1, 7])
@pytest.mark.parametrize("C,R,pieces", pc.GEOMETRIES)
def test_bad_rows(C, R, pieces, n_steps):
    pc.bad_rows("cuda", C, R, pieces, n_steps)


@pytest.mark.parametrize("null_arg", pc.GREEDY_ROWS_OPTIONAL)
@pytest.mark.parametrize("n", pc.FOOTPRINT_BATCHES)
@pytest.mark.parametrize("C,R", FOOT_GEOMETRIES)
def test_footprint_greedy_rows(C, R, n, null_arg):
    pc.footprint_greedy_rows("cuda", C, R, n, null_arg)


@pytest.mark.parametrize("null_arg", pc.PLAY_OPTIONAL)
@pytest.mark.parametrize("n", pc.FOOTPRINT_BATCHES)
@pytest.mark.parametrize("C,R", FOOT_GEOMETRIES)
def test_footprint_play(C, R, n, null_arg):
    pc.footprint_play("cuda", C, R, n, null_arg)


def test_facade():
    pc.facade("cuda")
