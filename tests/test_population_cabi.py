"""CPU-only: tetris_hip_policy_greedy_rows and tetris_hip_play_linear refuse bad arguments with the code
include/tetris_hip.h names, before any launch, in the real library (no GPU is needed: it returns first) and in the
CPU harness (the same text, csrc/tetris_abi.inc).  Every pointer of a refused call is one address nothing may touch."""
import ctypes

import pytest

E_NULL, E_DESC, E_BATCH = -1, -2, -6  # include/tetris_hip.h


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
    import harness_backend
    return harness_backend.binding()


def _refused_calls(d, z, p):
    """(label, entry, arguments, code).  d: a 10x20 descriptor, z: a zeroed one, p: a valid address nothing may read
    or write."""
    rows = []

    def vary(entry, good, changes):
        for label, at, value, code in changes:
            args = list(good)
            for a, v in zip(at if isinstance(at, tuple) else (at,), value if isinstance(at, tuple) else (value,)):
                args[a] = v
            rows.append(("%s: %s" % (entry, label), entry, args, code))

    nulls = lambda names: [("%s NULL" % n, at, None, E_NULL) for n, at in names]
    # desc cols meta weights P rows best_action best_value status B hip_stream
    vary("policy_greedy_rows", [d, p, p, p, 7, p, p, None, None, 16, None],
         nulls([("desc", 0), ("cols", 1), ("meta", 2), ("weights", 3), ("best_action", 6)]) +
         [("zeroed descriptor", 0, z, E_DESC), ("B = 0", 9, 0, E_BATCH), ("B < 0", 9, -1, E_BATCH),
          ("B past the 32-bit byte offsets", 9, 1 << 26, E_BATCH), ("P = 0", 4, 0, E_BATCH), ("P < 0", 4, -3, E_BATCH),
          ("no rows and P < B", 5, None, E_BATCH), ("no rows and P = B - 1", (4, 5), (15, None), E_BATCH)])
    # desc cols meta n_steps weights P rows lines_total pieces_total n_valid piece status seed step_idx0 env_offset B
    vary("play_linear", [d, p, p, 4, p, 7, p, p, p, None, None, None, 0, 0, 0, 16, None],
         nulls([("desc", 0), ("cols", 1), ("meta", 2), ("weights", 4), ("lines_total", 7), ("pieces_total", 8)]) +
         [("zeroed descriptor", 0, z, E_DESC), ("B = 0", 15, 0, E_BATCH), ("B < 0", 15, -1, E_BATCH),
          ("B past the 32-bit byte offsets", 15, 1 << 26, E_BATCH), ("n_steps = 0", 3, 0, E_BATCH),
          ("n_steps < 0", 3, -1, E_BATCH), ("P = 0", 5, 0, E_BATCH), ("P < 0", 5, -3, E_BATCH),
          ("no rows and P < B", 6, None, E_BATCH), ("no rows and P = B - 1", (5, 6), (15, None), E_BATCH)])
    return rows


@pytest.mark.parametrize("which", ["hip", "host"])
def test_refused_calls_return_the_headers_code(which, hip_lib, host_lib):
    from tetris_amd import _lib
    lib = hip_lib if which == "hip" else host_lib
    d, z = _lib.TetrisDesc(), _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    guard = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    rows = _refused_calls(ctypes.byref(d), ctypes.byref(z), ctypes.addressof(guard))
    assert len({r[0] for r in rows}) == len(rows) == 29
    got = [(label, getattr(lib, entry)(*args), code) for label, entry, args, code in rows]
    assert [g for g in got if g[1] != g[2]] == []
    assert guard.raw == b"\xa5" * 64  # nothing was written


def test_accepted_calls_get_past_the_checks(host_lib):
    """P = B without rows, and rows with P = 1, pass every check of the text.  Harness only (a call that passes
    its checks runs): it is the same text in the library."""
    from tetris_amd import _lib
    lib = host_lib
    d = _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    n = 3
    cols, meta = (ctypes.c_uint32 * 512)(), (ctypes.c_uint64 * n)()
    weights, rows = (ctypes.c_float * (8 * n))(), (ctypes.c_int32 * n)()
    best, lines, pieces = ((ctypes.c_int32 * n)() for _ in range(3))
    a = ctypes.addressof
    assert lib.reset(ctypes.byref(d), a(cols), a(meta), None, None, None, None, None, 0, None, 1, 0, 0, 0, n, None) == 0
    assert lib.policy_greedy_rows(ctypes.byref(d), a(cols), a(meta), a(weights), n, None, a(best), None, None, n, None) == 0
    assert lib.policy_greedy_rows(ctypes.byref(d), a(cols), a(meta), a(weights), 1, a(rows), a(best), None, None, n, None) == 0
    assert list(best) == [0] * n  # zero weights on an empty board: every placement ties, the lowest index wins
    assert lib.play_linear(ctypes.byref(d), a(cols), a(meta), 2, a(weights), n, None, a(lines), a(pieces), None, None, None,
                           0, 0, 0, n, None) == 0
    assert list(pieces) == [2] * n


def test_signatures_and_version(hip_lib, host_lib):
    from tetris_amd import _lib
    for name in ("tetris_hip_policy_greedy_rows", "tetris_hip_play_linear"):
        assert name in _lib.SIGNATURES and hasattr(hip_lib.cdll, name)
        assert hasattr(host_lib.cdll, "tetris_host_" + name[len("tetris_hip_"):])
    assert _lib.ABI_VERSION == 7 == hip_lib.version() == host_lib.version()
