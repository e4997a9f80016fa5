"""The two-piece lookahead on the MI355X: two_ply_kernel through the C-ABI (tests/two_ply_cases.py has the cases)."""
import numpy as np
import pytest

import two_ply_cases as tp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from tetris_amd import _lib
    old = _lib._install_test_backend(None)  # the real library, whatever a test before this module bound
    try:
        return _lib.load()
    finally:
        _lib._install_test_backend(old)


@pytest.mark.parametrize("C,R,pieces", tp.TABLE_GEOMETRIES)
def test_table_vs_oracle(lib, orc, C, R, pieces):
    tp.table_vs_oracle("cuda", orc, C, R, pieces)


def test_sums_and_pick(lib):
    tp.sums_and_pick("cuda")


@pytest.mark.parametrize("C,R,pieces", [(10, 20, "default"), (10, 40, tp.gc.STANDARD7), (12, 59, "default")])
def test_position_independence(lib, C, R, pieces):
    tp.position_independence("cuda", C, R, pieces)


def test_many_workgroups(lib):
    tp.many_workgroups("cuda")


@pytest.mark.parametrize("form", tp.FOOTPRINT_FORMS)
@pytest.mark.parametrize("B", tp.fc.ROLLOUT_BATCHES)
@pytest.mark.parametrize("C,R", tp.fc.GEOMETRIES)
def test_footprint(lib, C, R, B, form):
    tp.footprint(lib, "cuda", C, R, B, form)


def test_plays(lib, golden_dir):
    """every action is the NumPy pick on that round's two_ply_values; the trace is the CPU harness's"""
    np.testing.assert_array_equal(tp.plays("cuda"), tp.stored_trace(golden_dir))


def test_replay_mode(lib):
    tp.replay_mode("cuda")
