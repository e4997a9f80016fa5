"""Writes g12_two_ply_trace.npy: the action trace of two_ply_cases.plays on the CPU harness (int8 [40, 64]).
Run from the repository root after building the harness: python tests/golden/make_golden_two_ply.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

if __name__ == "__main__":
    import harness_backend
    import two_ply_cases as tp
    from tetris_amd import _lib
    _lib._install_test_backend(harness_backend.binding())
    trace = tp.plays("cpu")
    np.save(os.path.join(HERE, tp.TRACE_FILE), trace)
    print(trace.shape, trace.dtype, int(trace.min()), int(trace.max()))
