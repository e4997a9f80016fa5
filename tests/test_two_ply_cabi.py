"""CPU-only: tetris_hip_policy_two_ply refuses bad arguments with the code include/tetris_hip.h names, before any launch
and without writing anything, in the real library (no GPU is needed: it returns first) and in the CPU harness (the same
text, csrc/tetris_abi.inc); the header's declaration agrees with the ctypes signature argument by argument."""
import ctypes
import os
import re

import pytest

E_NULL, E_DESC, E_BATCH, E_VALUE = -1, -2, -6, -12  # include/tetris_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tetris_hip_policy_two_ply"
WEIGHTS = (ctypes.c_float * 8)(-24.04, -19.77, -13.08, -12.63, -10.49, -9.22, 6.6, -1.61)


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


def _rows(d, z, base):
    """(label, arguments, code).  cols, meta and the five outputs are ADDRESSES nothing may dereference: a refused call
    that wrote or read through one of them would fault."""
    cols, meta = base, base + (1 << 20)
    o = [base + k * (1 << 20) for k in range(2, 7)]
    w = ctypes.cast(WEIGHTS, ctypes.c_void_p)
    # desc cols meta weights death_value values q n_bag best_action best_value B hip_stream
    good = [d, cols, meta, w, -1000.0] + o + [100, None]
    rows = []

    def vary(label, at, value, code):
        args = list(good)
        args[at] = value
        rows.append((label, args, code))

    for name, at in (("desc", 0), ("cols", 1), ("meta", 2), ("weights", 3)):
        vary("%s NULL" % name, at, None, E_NULL)
    vary("zeroed descriptor", 0, z, E_DESC)
    vary("B = 0", 10, 0, E_BATCH)
    vary("B < 0", 10, -1, E_BATCH)
    vary("B past the 32-bit byte offsets", 10, 1 << 26, E_BATCH)
    vary("death_value NaN", 4, float("nan"), E_VALUE)
    vary("death_value +inf", 4, float("inf"), E_VALUE)
    return rows


@pytest.mark.parametrize("which", ["hip", "host"])
def test_refusals(which, hip_lib, host_lib):
    from tetris_amd import _lib
    lib = hip_lib if which == "hip" else host_lib
    d, z = _lib.TetrisDesc(), _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    rows = _rows(ctypes.byref(d), ctypes.byref(z), 1 << 40)
    assert len({r[0] for r in rows}) == len(rows) == 10
    got = [(label, lib.policy_two_ply(*args), code) for label, args, code in rows]
    assert [g for g in got if g[1] != g[2]] == []


@pytest.mark.parametrize("which", ["hip", "host"])
@pytest.mark.parametrize("death_value", [-float("inf"), -1000.0, 0.0, 3.0e38, -3.0e38])
def test_all_outputs_null_is_a_no_op(which, hip_lib, host_lib, death_value):
    """every accepted death_value; cols and meta are addresses nothing may read: the call returns 0 without a launch"""
    from tetris_amd import _lib
    lib = hip_lib if which == "hip" else host_lib
    d = _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    assert lib.policy_two_ply(ctypes.byref(d), 1 << 40, 1 << 41, ctypes.cast(WEIGHTS, ctypes.c_void_p), death_value,
                              None, None, None, None, None, 100, None) == 0


def test_refused_calls_write_nothing(host_lib):
    """real buffers on the harness (a call that passes its checks runs there): a refused death_value leaves them alone"""
    from tetris_amd import _lib
    lib = host_lib
    d = _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    cols, meta = (ctypes.c_uint32 * 512)(), (ctypes.c_uint64 * 64)()
    ad = ctypes.addressof
    assert lib.reset(ctypes.byref(d), ad(cols), ad(meta), None, None, None, None, None, 0, None, 1, 0, 0, 0, 64, None) == 0
    A, P = d.a_max, d.n_pieces
    values, q = (ctypes.c_uint32 * (3 * A * P))(*([7] * (3 * A * P))), (ctypes.c_uint32 * (3 * A))(*([7] * (3 * A)))
    n_bag, act, val = (ctypes.c_uint8 * 3)(7, 7, 7), (ctypes.c_int32 * 3)(7, 7, 7), (ctypes.c_uint32 * 3)(7, 7, 7)
    args = lambda dv: (ctypes.byref(d), ad(cols), ad(meta), ctypes.cast(WEIGHTS, ctypes.c_void_p), dv, ad(values), ad(q), ad(n_bag),
                       ad(act), ad(val), 3, None)
    assert lib.policy_two_ply(*args(float("nan"))) == E_VALUE
    assert set(values) == set(q) == set(n_bag) == set(act) == set(val) == {7}
    assert lib.policy_two_ply(*args(-float("inf"))) == 0
    assert list(n_bag) == [1, 1, 1]  # (a fresh bag of two after the reset's draw)
    assert all(0 <= a < A for a in act) and 7 not in set(q)


def test_signature_version_and_error_string(hip_lib, host_lib):
    from tetris_amd import _lib
    assert NAME in _lib.SIGNATURES and NAME in _lib.EXPORTS and hasattr(hip_lib.cdll, NAME)
    assert hasattr(host_lib.cdll, "tetris_host_policy_two_ply")
    assert _lib.ABI_VERSION == 7 == hip_lib.version() == host_lib.version()
    for lib in (hip_lib, host_lib):
        assert "death_value" in lib.error_string(E_VALUE)


def test_header_text_matches_the_binding():
    """the declaration of include/tetris_hip.h, argument by argument, against the ctypes signature"""
    from tetris_amd import _lib
    header = open(os.path.join(ROOT, "include", "tetris_hip.h")).read()
    kinds = {ctypes.c_void_p: "pointer", ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t", ctypes.c_uint64: "uint64_t",
             ctypes.c_float: "float", _lib._dp: "pointer"}
    m = re.search(r"\bint %s\(([^;]*)\);" % NAME, header)
    assert m
    declared, names = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        declared.append("pointer" if "*" in arg else arg.rsplit(" ", 1)[0].replace("const ", ""))
        names.append(arg.rsplit(" ", 1)[1].lstrip("*"))
    assert declared == [kinds[t] for t in _lib.SIGNATURES[NAME]]
    assert names == ["desc", "cols", "meta", "weights", "death_value", "values", "q", "n_bag", "best_action", "best_value", "B",
                     "hip_stream"]
    assert "#define TETRIS_HIP_ABI_VERSION 7" in header and "TETRIS_E_VALUE = %d" % E_VALUE in header
