"""CPU-only checks of the boundary: the C-ABI library loads without a GPU and exports every
symbol include/tetris_hip.h declares; argument errors come back as codes before any launch;
the host-side tables agree with the library."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip_lib():
    from tetris_amd import _lib
    old = _lib._install_test_backend(None)  # make sure the real library is what load() returns
    try:
        b = _lib.load()
    finally:
        _lib._install_test_backend(old)
    return b


@pytest.fixture(scope="module")
def host_lib():
    """The CPU harness: the same C-ABI text (csrc/tetris_abi.inc) on loops over envs, prefix tetris_host_."""
    import harness_backend
    return harness_backend.binding()


def test_header_symbols_are_exported(hip_lib, host_lib):
    header = open(os.path.join(ROOT, "include", "tetris_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(tetris_hip_\w+)\s*\(", header)))
    assert len(declared) >= 12
    for name in declared:
        assert hasattr(hip_lib.cdll, name), "libtetris_hip.so does not export %s" % name
        host_name = "tetris_host_" + name[len("tetris_hip_"):]
        assert hasattr(host_lib.cdll, host_name), "libtetris_core_host.so does not export %s" % host_name
    from tetris_amd import _lib
    assert set(_lib.EXPORTS) == set(declared)
    assert hip_lib.version() == _lib.ABI_VERSION == host_lib.version()


def test_step_call_size_agrees(hip_lib, host_lib):
    """Both libraries bind a step in the same struct (TetrisStepCall, csrc/tetris_entry.hpp)."""
    assert hip_lib.step_call_size() == host_lib.step_call_size() > 0


E_NULL, E_DESC, E_PIECES, E_BATCH, E_STREAM, E_STRIDE = -1, -2, -5, -6, -7, -8  # include/tetris_hip.h


def _refused_calls(d, z, p, call, zero_call):
    """(label, entry, arguments, code the header names).  d: a 10x20 descriptor, z: a zeroed one, p: a valid
    address nothing may read or write, call: room for a bound call (a refused init leaves it unbound), zero_call:
    step_call_size() zero bytes (no bound call).  Every row fails a check of csrc/tetris_abi.inc, so neither library
    gets as far as its backend (the real one: a launch)."""
    rows = []

    def vary(entry, good, changes):
        for label, at, value, code in changes:
            args = list(good)
            for a, v in zip(at if isinstance(at, tuple) else (at,), value if isinstance(at, tuple) else (value,)):
                args[a] = v
            rows.append(("%s: %s" % (entry, label), entry, args, code))

    batch = lambda at: [("B = 0", at, 0, E_BATCH), ("B < 0", at, -1, E_BATCH)]
    nulls = lambda names: [("%s NULL" % n, at, None, E_NULL) for n, at in names]
    streams = lambda s, c, n: [("stream without cursor", (s, c, n), (p, None, 4), E_STREAM),
                               ("stream_len = 0", (s, c, n), (p, p, 0), E_STREAM)]
    # desc cols meta action action_out stream cursor stream_len obs reward done lines n_valid_next piece_next status
    # auto_reset seed step_idx env_offset B hip_stream
    vary("step", [d, p, p, None, None, None, None, 0, None, p, p, p, p, None, None, 0, 0, 0, 0, 16, None],
         nulls([("cols", 1), ("meta", 2), ("reward", 9), ("done", 10), ("lines", 11), ("n_valid_next", 12)]) + batch(19) +
         [("zeroed descriptor", 0, z, E_DESC), ("B past the 32-bit byte offsets", 19, 1 << 26, E_BATCH)] + streams(5, 6, 7))
    # desc cols meta reset_mask piece_out n_valid_out stream cursor stream_len status init_bag seed step_idx env_offset B
    vary("reset", [d, p, p, None, None, None, None, None, 0, None, 1, 0, 0, 0, 16, None],
         nulls([("cols", 1), ("meta", 2)]) + batch(14) + [("zeroed descriptor", 0, z, E_DESC)] + streams(6, 7, 8))
    # call desc cols meta action_out stream cursor stream_len obs reward done lines n_valid_next piece_next status
    # auto_reset seed env_offset B
    vary("step_call_init", [call, d, p, p, None, None, None, 0, None, p, p, p, p, None, None, 0, 0, 0, 16],
         nulls([("call", 0), ("cols", 2), ("n_valid_next", 12)]) + batch(18) + [("zeroed descriptor", 1, z, E_DESC)] +
         streams(5, 6, 7))
    # desc cols meta feats n_valid feats_all n_all env_stride row_stride B
    vary("afterstates", [d, p, p, p, p, None, None, 288, 8, 16, None],
         nulls([("cols", 1), ("meta", 2), ("feats", 3), ("n_valid", 4)]) + batch(9) +
         [("zeroed descriptor", 0, z, E_DESC), ("row_stride 4", 8, 4, E_STRIDE), ("row_stride 6", 8, 6, E_STRIDE),
          ("env_stride 4", 7, 4, E_STRIDE), ("env_stride 6", 7, 6, E_STRIDE),
          ("env_stride not a multiple of 4", 7, 290, E_STRIDE), ("matrix beyond 2^32 float4", 9, 1 << 40, E_STRIDE)])
    # desc cols meta n_steps policy weights action_out obs reward done lines n_valid_next piece_next status auto_reset
    # seed step_idx0 env_offset B
    vary("step_many", [d, p, p, 4, 0, None, None, None, p, p, p, p, None, None, 0, 0, 0, 0, 16, None],
         nulls([("cols", 1), ("reward", 8)]) + batch(18) +
         [("zeroed descriptor", 0, z, E_DESC), ("n_steps = 0", 3, 0, E_BATCH), ("policy = 2", 4, 2, E_BATCH),
          ("greedy without weights", 4, 1, E_BATCH), ("B * n_steps over the limit", (3, 18), (64, 1 << 20), E_BATCH)])
    # desc cols meta returns length n policy weights pieces seed step_idx env_offset B
    vary("rollouts", [d, p, p, p, 3, 2, 0, None, None, 0, 0, 0, 16, None],
         nulls([("cols", 1), ("meta", 2), ("returns", 3)]) + batch(12) +
         [("zeroed descriptor", 0, z, E_DESC), ("length = 0", 4, 0, E_BATCH), ("n = 0", 5, 0, E_BATCH),
          ("policy = 2", 6, 2, E_BATCH), ("greedy without weights", 6, 1, E_NULL)])
    # desc cols meta weights best_action best_value fitness_all B
    vary("policy_greedy", [d, p, p, p, p, None, None, 16, None],
         nulls([("cols", 1), ("meta", 2), ("weights", 3), ("best_action", 4)]) + batch(7) +
         [("zeroed descriptor", 0, z, E_DESC)])
    vary("refresh", [d, p, p, None, 16, None],
         nulls([("cols", 1), ("meta", 2)]) + batch(4) + [("zeroed descriptor", 0, z, E_DESC)])
    vary("policy_random", [p, p, 0, 0, 0, 16, None], nulls([("n_valid", 0), ("action", 1)]) + batch(5))
    # seeds n_pieces L stream B
    vary("numpy_bag_stream", [p, 2, 8, p, 16, None],
         nulls([("seeds", 0), ("stream", 3)]) + batch(4) +
         [("n_pieces = 0", 1, 0, E_PIECES), ("n_pieces = 13", 1, 13, E_PIECES), ("L = 0", 2, 0, E_BATCH)])
    vary("decode", [d, p, p, None, 16, None], nulls([("cols", 1)]) + batch(4) + [("zeroed descriptor", 0, z, E_DESC)])
    vary("encode", [d, p, p, 16, None],
         nulls([("cells", 1), ("cols", 2)]) + batch(3) + [("zeroed descriptor", 0, z, E_DESC)])
    vary("pack_done_bits", [p, p, 16, None], nulls([("done", 0), ("bits", 1)]) + batch(2))
    vary("counter_add", [p, 1, None], nulls([("counter", 0)]))
    vary("board_words", [d, 16], batch(1) + [("zeroed descriptor", 0, z, E_DESC)])
    vary("n_planes", [d], [("zeroed descriptor", 0, z, E_DESC)])
    vary("n_placements", [0, 10], [("catalogue id -1", 0, -1, E_PIECES), ("catalogue id 9", 0, 9, E_PIECES)])
    no_call = [("NULL call", 0, None, E_NULL), ("zero-filled call", 0, zero_call, E_DESC)]
    vary("step_call_run", [p, None, 0, None], no_call)
    vary("step_call_run_gather", [p, None, 0, None, None, None], no_call)
    vary("step_call_run_counted", [p, None, p, 0, None], no_call + [("NULL counter", (0, 2), (zero_call, None), E_NULL)])
    return rows


@pytest.mark.parametrize("which", ["hip", "host"])
def test_refused_calls_return_the_headers_code(which, hip_lib, host_lib):
    """One table of calls the C-ABI must refuse, against the real library (which returns before any launch: no GPU
    is needed) and against the CPU harness: the same text, so the same code from both."""
    from tetris_amd import _lib
    lib = hip_lib if which == "hip" else host_lib
    d, z = _lib.TetrisDesc(), _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    guard = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    call, zero_call = (ctypes.create_string_buffer(lib.step_call_size()) for _ in range(2))
    rows = _refused_calls(ctypes.byref(d), ctypes.byref(z), ctypes.addressof(guard), ctypes.addressof(call),
                          ctypes.addressof(zero_call))
    assert len(rows) > 100 and len({r[0] for r in rows}) == len(rows)
    got = [(label, getattr(lib, entry)(*args), code) for label, entry, args, code in rows]
    assert [g for g in got if g[1] != g[2]] == []
    assert guard.raw == b"\xa5" * 64 and zero_call.raw == bytes(len(zero_call))  # nothing was written


def test_desc_init_and_argument_errors(hip_lib):
    from tetris_amd import _lib
    d = _lib.TetrisDesc()
    ids = (ctypes.c_int32 * 2)(4, 3)
    assert hip_lib.desc_init(ctypes.byref(d), 10, 20, ids, 2, None) == 0
    assert (d.word_bytes, d.a_max, d.n_pieces) == (4, 36, 2)
    assert hip_lib.desc_init(ctypes.byref(d), 10, 40, ids, 2, None) == 0 and d.word_bytes == 8
    assert hip_lib.desc_init(ctypes.byref(d), 13, 20, ids, 2, None) == -3     # TETRIS_E_COLUMNS (5..12 are built)
    assert hip_lib.desc_init(ctypes.byref(d), 4, 20, ids, 2, None) == -3
    assert hip_lib.desc_init(ctypes.byref(d), 10, 3, ids, 2, None) == -4      # TETRIS_E_ROWS
    assert hip_lib.desc_init(ctypes.byref(d), 10, 20, ids, 0, None) == -5     # TETRIS_E_PIECES
    bad = (ctypes.c_int32 * 1)(9)
    assert hip_lib.desc_init(ctypes.byref(d), 10, 20, bad, 1, None) == -5
    assert hip_lib.desc_init(ctypes.byref(d), 10, 20, ids, 2, None) == 0
    # NULL pointers / bad batch are refused before anything is launched (no GPU needed)
    assert hip_lib.step(ctypes.byref(d), None, None, None, None, None, None, 0, None, None, None, None, None, None,
                        None, 0, 0, 0, 0, 16, None) == -1
    assert hip_lib.reset(ctypes.byref(d), None, None, None, None, None, None, None, 0, None, 1, 0, 0, 0, 16, None) == -1
    z = _lib.TetrisDesc()
    assert hip_lib.refresh(ctypes.byref(z), None, None, None, 16, None) == -2  # uninitialised descriptor
    assert "NULL" in hip_lib.error_string(-1)
    cols = (ctypes.c_int32 * 16)()
    n = hip_lib.supported_columns(cols, 16)
    assert list(cols)[:n] == [5, 6, 7, 8, 9, 10, 11, 12]
    from tetris_amd import build
    assert list(build._COLUMNS) == list(cols)[:n]  # the per-column translation units of the in-tree build
    assert hip_lib.status_words(1 << 20) == 4 * ((1 << 20) // 64)


def test_host_tables_match_library(hip_lib):
    from tetris_amd.tetromino import CATALOGUE, ORIENTATIONS, n_placements
    want = dict(Straight=17, Square=9, SnakeR=17, ThreeLine=18, ThreeL=36, SnakeL=17, T=34, RCorner=34, LCorner=34)
    for i, name in enumerate(CATALOGUE):
        for C in (5, 6, 7, 8, 9, 10):
            assert hip_lib.n_placements(i, C) == n_placements(name, C)
        assert n_placements(name, 10) == want[name]
        for loop in ORIENTATIONS[name]:
            for w, b, n in loop:
                assert len(b) == len(n) == w and min(b) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No CPU fallback: without the HIP extension (and without hipcc) the package refuses to work."""
    from tetris_amd import _lib, build
    old = _lib._install_test_backend(None)
    try:
        monkeypatch.setattr(build, "SO_PATH", str(tmp_path / "nope.so"))
        monkeypatch.setattr(build, "_hipcc", lambda: (_ for _ in ()).throw(RuntimeError("no hipcc")))
        with pytest.raises(ImportError):
            _lib.load()
    finally:
        _lib._install_test_backend(old)


def test_vec_env_rejects_cpu_device_without_test_backend():
    from tetris_amd import VecTetris, _lib
    old = _lib._install_test_backend(None)
    try:
        with pytest.raises(ValueError):
            VecTetris(10, 20, 4, device="cpu")
    finally:
        _lib._install_test_backend(old)


def test_done_bit_packing_roundtrip():
    import torch
    from tetris_amd.distributed import pack_done_bits, shard_range, unpack_done_bits
    d = torch.rand(1003) < 0.1
    bits = pack_done_bits(d)
    assert bits.numel() == 126 and torch.equal(unpack_done_bits(bits, 1003), d)
    assert shard_range(1 << 23, 3, 8) == (3 << 20, 4 << 20)
    with pytest.raises(ValueError):
        shard_range(10, 0, 3)
