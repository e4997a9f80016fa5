"""Expanding envs into their afterstates on the MI355X: expand_kernel through the C-ABI."""
import pytest

import expand_cases as ec
import gather_cases as gc

pytestmark = pytest.mark.gpu

GOLDEN = ["g1_placements_10x20.npz", "g1_placements_10x40.npz", "g1_placements_6x10.npz", "g1_placements_12x20.npz"]


@pytest.fixture(scope="module")
def lib():
    from tetris_amd import _lib
    old = _lib._install_test_backend(None)  # the real library, whatever a test before this module bound
    try:
        return _lib.load()
    finally:
        _lib._install_test_backend(old)


@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_children_vs_oracle(orc, C, R, pieces):
    ec.children_vs_oracle("cuda", orc, C, R, pieces)


@pytest.mark.parametrize("fname", GOLDEN)
def test_children_vs_golden(golden_dir, fname):
    ec.children_vs_golden("cuda", golden_dir, fname)


@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_drawn_equals_step(C, R, pieces):
    ec.drawn_equals_step("cuda", C, R, pieces)


@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_drawn_equals_step_partial_tiles(C, R, pieces):
    ec.drawn_equals_step("cuda", C, R, pieces, B_src=200, B_dst=321)


def test_drawn_equals_step_many_workgroups():
    """258 workgroups of dst, parents from all over 1025 src tiles: partial last tiles on both sides"""
    ec.drawn_equals_step("cuda", 10, 20, "default", B_src=65573, B_dst=66001)


@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_repeated_parents_share_the_piece(C, R, pieces):
    ec.repeated_parents_share_the_piece("cuda", C, R, pieces)


def test_shard_draws_the_batchs_pieces():
    ec.shard_draws_the_batchs_pieces("cuda", 10, 20, gc.STANDARD7)


@pytest.mark.parametrize("B_dst", gc.B_DSTS)
@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_untouched_and_invalid(C, R, pieces, B_dst):
    ec.untouched_and_invalid("cuda", C, R, pieces, B_dst)


@pytest.mark.parametrize("with_optional", [True, False])
@pytest.mark.parametrize("B", gc.B_DSTS)
@pytest.mark.parametrize("C,R", ec.fc.GEOMETRIES)
def test_footprint(lib, C, R, B, with_optional):
    ec.footprint(lib, "cuda", C, R, B, with_optional)


def test_host_refusals():
    ec.host_refusals("cuda")


@pytest.mark.parametrize("C,R,pieces", ec.GEOMETRIES)
def test_child_is_an_env(C, R, pieces):
    ec.child_is_an_env("cuda", C, R, pieces)


@pytest.mark.parametrize("C,R", [(6, 10), (10, 20)])
def test_two_ply_vs_oracle(orc, C, R):
    ec.two_ply_vs_oracle("cuda", orc, C, R)
