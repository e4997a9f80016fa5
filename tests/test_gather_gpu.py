"""Copying envs between batches by index on the MI355X: gather_envs_kernel through the C-ABI."""
import pytest

import gather_cases as gc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B_dst", gc.B_DSTS)
@pytest.mark.parametrize("C,R,pieces", gc.GEOMETRIES)
def test_copy_is_exact(C, R, pieces, B_dst):
    gc.copy_is_exact("cuda", C, R, pieces, gc.B_SRC, B_dst)


def test_copy_is_exact_many_workgroups():
    """258 workgroups of dst, src tiles from all over 1025: partial last tiles on both sides"""
    gc.copy_is_exact("cuda", 10, 20, "default", 65573, 66001)


@pytest.mark.parametrize("C,R,pieces", gc.GEOMETRIES)
def test_bag_travels(C, R, pieces):
    gc.bag_travels("cuda", C, R, pieces)


@pytest.mark.parametrize("B_dst", gc.B_DSTS)
@pytest.mark.parametrize("C,R,pieces", gc.GEOMETRIES)
def test_out_of_range_entries(C, R, pieces, B_dst):
    gc.out_of_range_entries("cuda", C, R, pieces, gc.B_SRC, B_dst)


@pytest.mark.parametrize("C,R,pieces", gc.GEOMETRIES)
def test_gather_in_place(C, R, pieces):
    gc.gather_in_place("cuda", C, R, pieces)


def test_host_refusals():
    gc.host_refusals("cuda")
