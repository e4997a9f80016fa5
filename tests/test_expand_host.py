"""Expanding envs into their afterstates on CPU (harness backend): the per-env body the kernel runs, and the host
logic of expand_from / expand / two_ply_values."""
import pytest

import expand_cases as ec
import gather_cases as gc

GOLDEN = ["g1_placements_10x20.npz", "g1_placements_10x40.npz", "g1_placements_6x10.npz", "g1_placements_12x20.npz"]


@pytest.fixture(scope="module")
def lib():
    import harness_backend
    return harness_backend.binding()


@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_children_vs_oracle(host_backend, orc, C, R, pieces):
    ec.children_vs_oracle("cpu", orc, C, R, pieces)


@pytest.mark.parametrize("fname", GOLDEN)
def test_children_vs_golden(host_backend, golden_dir, fname):
    ec.children_vs_golden("cpu", golden_dir, fname)


@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_drawn_equals_step(host_backend, C, R, pieces):
    ec.drawn_equals_step("cpu", C, R, pieces)


@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_drawn_equals_step_partial_tiles(host_backend, C, R, pieces):
    ec.drawn_equals_step("cpu", C, R, pieces, B_src=200, B_dst=321)


@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_repeated_parents_share_the_piece(host_backend, C, R, pieces):
    ec.repeated_parents_share_the_piece("cpu", C, R, pieces)


def test_shard_draws_the_batchs_pieces(host_backend):
    ec.shard_draws_the_batchs_pieces("cpu", 10, 20, gc.STANDARD7)


@pytest.mark.parametrize("B_dst", gc.B_DSTS)
@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_untouched_and_invalid(host_backend, C, R, pieces, B_dst):
    ec.untouched_and_invalid("cpu", C, R, pieces, B_dst)


@pytest.mark.parametrize("with_optional", [True, False])
@pytest.mark.parametrize("B", gc.B_DSTS)
@pytest.mark.parametrize("C,R", ec.fc.GEOMETRIES)
def test_footprint(lib, C, R, B, with_optional):
    ec.footprint(lib, "cpu", C, R, B, with_optional)


def test_host_refusals(host_backend):
    ec.host_refusals("cpu")


@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_child_is_an_env(host_backend, C, R, pieces):
    ec.child_is_an_env("cpu", C, R, pieces)


@pytest.mark.parametrize("C,R", [(6, 10), (10, 20)])
def test_two_ply_vs_oracle(host_backend, orc, C, R):
    ec.two_ply_vs_oracle("cpu", orc, C, R)
