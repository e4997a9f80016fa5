"""Copying envs between batches by index on CPU (harness backend): the per-env body the kernel runs, and the
host logic of copy_envs_from / fork / gather_."""
import pytest

import gather_cases as gc


@pytest.mark.parametrize("B_dst", gc.B_DSTS)
@pytest.mark.parametrize("C,R,pieces", gc.GEOMETRIES)
def test_copy_is_exact(host_backend, C, R, pieces, B_dst):
    gc.copy_is_exact("cpu", C, R, pieces, gc.B_SRC, B_dst)


@pytest.mark.parametrize("C,R,pieces", gc.GEOMETRIES)
def test_bag_travels(host_backend, C, R, pieces):
    gc.bag_travels("cpu", C, R, pieces)


@pytest.mark.parametrize("B_dst", gc.B_DSTS)
@pytest.mark.parametrize("C,R,pieces", gc.GEOMETRIES)
def test_out_of_range_entries(host_backend, C, R, pieces, B_dst):
    gc.out_of_range_entries("cpu", C, R, pieces, gc.B_SRC, B_dst)


@pytest.mark.parametrize("C,R,pieces", gc.GEOMETRIES)
def test_gather_in_place(host_backend, C, R, pieces):
    gc.gather_in_place("cpu", C, R, pieces)


def test_host_refusals(host_backend):
    gc.host_refusals("cpu")
