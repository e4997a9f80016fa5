"""CPU-only: tetris_hip_policy_softmax_rows and tetris_hip_play_softmax refuse bad arguments with the code
include/tetris_hip.h names, before any launch, in the real library (no GPU is needed: it returns first) and in the
CPU harness (the same text, csrc/tetris_abi.inc).  Every pointer of a refused call is one address nothing may touch."""
import ctypes
import os
import re

import pytest

E_NULL, E_DESC, E_BATCH, E_ALIGN, E_TEMPERATURE = -1, -2, -6, -10, -11  # include/tetris_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tetris_hip_policy_softmax_rows", "tetris_hip_play_softmax")


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
    """(label, entry, arguments, code).  d: a 10x20 descriptor, z: a zeroed one, p: a valid 16-byte aligned address
    nothing may read or write."""
    rows = []

    def vary(entry, good, changes):
        for label, at, value, code in changes:
            args = list(good)
            for a, v in zip(at if isinstance(at, tuple) else (at,), value if isinstance(at, tuple) else (value,)):
                args[a] = v
            rows.append(("%s: %s" % (entry, label), entry, args, code))

    nulls = lambda names: [("%s NULL" % n, at, None, E_NULL) for n, at in names]
    temperatures = lambda at: [("temperature %r" % t, at, t, E_TEMPERATURE)
                               for t in (0.0, -1.0, float("inf"), float("-inf"), float("nan"), 1e-45)]
    # desc cols meta weights P rows temperature action logp score logz logits status seed step_idx env_offset B stream
    vary("policy_softmax_rows", [d, p, p, p, 7, p, 1.0, p, p, None, None, None, None, 0, 0, 0, 16, None],
         nulls([("desc", 0), ("cols", 1), ("meta", 2), ("weights", 3), ("action", 7), ("logp", 8)]) +
         [("zeroed descriptor", 0, z, E_DESC), ("B = 0", 16, 0, E_BATCH), ("B < 0", 16, -1, E_BATCH),
          ("B past the 32-bit byte offsets", 16, 1 << 26, E_BATCH), ("P = 0", 4, 0, E_BATCH), ("P < 0", 4, -3, E_BATCH),
          ("no rows and P < B", 5, None, E_BATCH), ("no rows and P = B - 1", (4, 5), (15, None), E_BATCH),
          ("weights off by 4 bytes", 3, p + 4, E_ALIGN), ("weights off by 8 bytes", 3, p + 8, E_ALIGN),
          ("score off by 4 bytes", 9, p + 4, E_ALIGN)] + temperatures(6))
    # desc cols meta n_steps weights P rows temperature lines_total pieces_total logp_total score_total n_valid piece
    # status seed step_idx0 env_offset B stream
    vary("play_softmax", [d, p, p, 4, p, 7, p, 1.0, p, p, None, p, None, None, None, 0, 0, 0, 16, None],
         nulls([("desc", 0), ("cols", 1), ("meta", 2), ("weights", 4), ("lines_total", 8), ("pieces_total", 9),
                ("score_total", 11)]) +
         [("zeroed descriptor", 0, z, E_DESC), ("B = 0", 18, 0, E_BATCH), ("B < 0", 18, -1, E_BATCH),
          ("B past the 32-bit byte offsets", 18, 1 << 26, E_BATCH), ("n_steps = 0", 3, 0, E_BATCH),
          ("n_steps < 0", 3, -1, E_BATCH), ("P = 0", 5, 0, E_BATCH), ("P < 0", 5, -3, E_BATCH),
          ("no rows and P < B", 6, None, E_BATCH), ("no rows and P = B - 1", (5, 6), (15, None), E_BATCH),
          ("weights off by 4 bytes", 4, p + 4, E_ALIGN), ("score_total off by 8 bytes", 11, p + 8, E_ALIGN)] +
         temperatures(7))
    return rows


@pytest.mark.parametrize("which", ["hip", "host"])
def test_refused_calls_return_the_headers_code(which, hip_lib, host_lib):
    from tetris_amd import _lib
    lib = hip_lib if which == "hip" else host_lib
    d, z = _lib.TetrisDesc(), _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    raw = ctypes.create_string_buffer(b"\xa5" * 96, 96)
    guard = (ctypes.addressof(raw) + 15) & ~15
    rows = _refused_calls(ctypes.byref(d), ctypes.byref(z), guard)
    assert len({r[0] for r in rows}) == len(rows) == 23 + 25
    got = [(label, getattr(lib, entry)(*args), code) for label, entry, args, code in rows]
    assert [g for g in got if g[1] != g[2]] == []
    assert raw.raw == b"\xa5" * 96  # nothing was written
    assert "temperature" in lib.error_string(E_TEMPERATURE) and "aligned" in lib.error_string(E_ALIGN)


def test_accepted_calls_get_past_the_checks(host_lib):
    """P = B without rows, rows with P = 1 and every optional pointer NULL pass every check of the text.  Harness
    only (a call that passes its checks runs): it is the same text in the library."""
    from tetris_amd import _lib
    lib = host_lib
    d = _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    n = 3
    cols, meta = (ctypes.c_uint32 * 512)(), (ctypes.c_uint64 * n)()
    room = ctypes.create_string_buffer(32 * n + 32 * n + 16)
    weights = (ctypes.addressof(room) + 15) & ~15  # zero weights [n][8], then score_total [n][8], 16-byte aligned
    score_total = weights + 32 * n
    rows, action, lines, pieces = ((ctypes.c_int32 * n)() for _ in range(4))
    logp = (ctypes.c_float * n)()
    a = ctypes.addressof
    assert lib.reset(ctypes.byref(d), a(cols), a(meta), None, None, None, None, None, 0, None, 1, 0, 0, 0, n, None) == 0
    for P, r in ((n, None), (1, a(rows))):
        assert lib.policy_softmax_rows(ctypes.byref(d), a(cols), a(meta), weights, P, r, 1.0, a(action), a(logp), None, None,
                                       None, None, 0, 0, 0, n, None) == 0
        assert all(0 <= x < d.a_max for x in action)
        assert all(abs(x - logp[0]) < 1e-6 and x < 0 for x in logp)  # zero weights on empty boards: uniform
    assert lib.play_softmax(ctypes.byref(d), a(cols), a(meta), 2, weights, n, None, 0.5, a(lines), a(pieces), None,
                            score_total, None, None, None, 0, 0, 0, n, None) == 0
    assert list(pieces) == [2] * n


def test_signatures_and_version(hip_lib, host_lib):
    from tetris_amd import _lib
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(hip_lib.cdll, name)
        assert hasattr(host_lib.cdll, "tetris_host_" + name[len("tetris_hip_"):])
    assert _lib.ABI_VERSION == 7 == hip_lib.version() == host_lib.version()


def test_header_text_matches_the_binding():
    """the declarations of include/tetris_hip.h, argument by argument, against the ctypes signatures"""
    from tetris_amd import _lib
    header = open(os.path.join(ROOT, "include", "tetris_hip.h")).read()
    kinds = {ctypes.c_void_p: "pointer", ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t", ctypes.c_uint64: "uint64_t",
             ctypes.c_float: "float", _lib._dp: "pointer"}
    for name in NAMES:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        declared = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            declared.append("pointer" if "*" in arg else arg.rsplit(" ", 1)[0].replace("const ", ""))
        assert declared == [kinds[t] for t in _lib.SIGNATURES[name]], name
    assert "TETRIS_E_ALIGN = %d" % E_ALIGN in header and "TETRIS_E_TEMPERATURE = %d" % E_TEMPERATURE in header
    for phrase in ("0x9E3779B1u", "WITHOUT the factor 1 / temperature", "IN\n *          THE ORDER THE PLACEMENT WALK EMITS"):
        assert phrase in header, phrase
