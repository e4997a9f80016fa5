"""CPU-only: tetris_hip_expand_envs refuses bad arguments with the code include/tetris_hip.h names, before any launch,
in the real library (no GPU is needed: it returns first) and in the CPU harness (the same text, csrc/tetris_abi.inc);
and the header's declaration agrees with the ctypes signature argument by argument."""
import ctypes
import os
import re

import pytest

E_NULL, E_DESC, E_BATCH, E_OVERLAP = -1, -2, -6, -9  # include/tetris_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tetris_hip_expand_envs"


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
    """(label, arguments, code).  d: a 10x20 descriptor (8 planes of 4-byte words: 2048 B of cols per tile), z: a zeroed
    one.  The buffers are ADDRESSES nothing may dereference: 64 src envs (cols 2048 B, meta 512 B) and 100 dst envs
    (cols 4096 B, meta 800 B), far apart."""
    src_cols, src_meta, dst_cols, dst_meta = (base + k * (1 << 20) for k in range(4))
    o = [base + k * (1 << 20) for k in range(4, 14)]
    # desc src_cols src_meta B_src dst_cols dst_meta parent action next_piece obs reward done lines n_valid piece status
    # seed step_idx env_offset B_dst hip_stream
    good = [d, src_cols, src_meta, 64, dst_cols, dst_meta, o[0], o[1], None, None, o[4], o[5], o[6], o[7], o[8], None, 0, 0, 0,
            100, None]
    rows = []

    def vary(label, at, value, code):
        args = list(good)
        for a, v in zip(at if isinstance(at, tuple) else (at,), value if isinstance(at, tuple) else (value,)):
            args[a] = v
        rows.append((label, args, code))

    for name, at in (("desc", 0), ("src_cols", 1), ("src_meta", 2), ("dst_cols", 4), ("dst_meta", 5), ("parent", 6),
                     ("action", 7), ("reward", 10), ("done", 11), ("lines", 12), ("n_valid", 13), ("piece", 14)):
        vary("%s NULL" % name, at, None, E_NULL)
    vary("zeroed descriptor", 0, z, E_DESC)
    for name, at in (("B_src", 3), ("B_dst", 19)):
        vary("%s = 0" % name, at, 0, E_BATCH)
        vary("%s < 0" % name, at, -1, E_BATCH)
        vary("%s past the 32-bit byte offsets" % name, at, 1 << 26, E_BATCH)
    vary("dst_cols == src_cols", 4, src_cols, E_OVERLAP)
    vary("dst_cols begins in the last word of src_cols", 4, src_cols + 2048 - 4, E_OVERLAP)
    vary("dst_cols ends in the first word of src_cols", 4, src_cols - 4096 + 4, E_OVERLAP)
    vary("dst_meta == src_meta", 5, src_meta, E_OVERLAP)
    vary("dst_meta begins in the last word of src_meta", 5, src_meta + 512 - 8, E_OVERLAP)
    vary("dst_meta ends in the first word of src_meta", 5, src_meta - 800 + 8, E_OVERLAP)
    vary("both overlap", (4, 5), (src_cols, src_meta), E_OVERLAP)
    return rows


@pytest.mark.parametrize("which", ["hip", "host"])
def test_expand_envs_refusals(which, hip_lib, host_lib):
    from tetris_amd import _lib
    lib = hip_lib if which == "hip" else host_lib
    d, z = _lib.TetrisDesc(), _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    assert lib.n_planes(ctypes.byref(d)) == 8 and d.word_bytes == 4
    rows = _rows(ctypes.byref(d), ctypes.byref(z), 1 << 40)
    assert len({r[0] for r in rows}) == len(rows) == 26
    got = [(label, lib.expand_envs(*args), code) for label, args, code in rows]
    assert [g for g in got if g[1] != g[2]] == []


def test_optional_pointers_and_adjacent_storage(host_lib):
    """next_piece, obs and status NULL, dst right behind src: the call gets past every check of the text and runs.
    Harness only (a call that passes its checks runs): it is the same text in the library."""
    from tetris_amd import _lib
    lib = host_lib
    d = _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    cols = (ctypes.c_uint32 * (2 * 512))()   # src tile | dst tile
    meta = (ctypes.c_uint64 * (2 * 64))()
    a, m = ctypes.addressof(cols), ctypes.addressof(meta)
    assert lib.reset(ctypes.byref(d), a, m, None, None, None, None, None, 0, None, 1, 0, 0, 0, 64, None) == 0
    parent = (ctypes.c_int32 * 64)(*([-1] * 62 + [3, 64]))
    action = (ctypes.c_int32 * 64)()
    reward = (ctypes.c_int32 * 64)(*([77] * 64))
    done, lines, n_valid, piece = ((ctypes.c_uint8 * 64)(*([9] * 64)) for _ in range(4))
    ad = ctypes.addressof
    assert lib.expand_envs(ctypes.byref(d), a, m, 64, a + 2048, m + 512, ad(parent), ad(action), None, None, ad(reward), ad(done),
                           ad(lines), ad(n_valid), ad(piece), None, 0, 0, 0, 64, None) == 0
    assert list(reward) == [77] * 62 + [-1, 77] and list(done) == [9] * 62 + [0, 9] and list(lines) == [9] * 62 + [0, 9]
    assert piece[62] in (0, 1) and 0 < n_valid[62] <= d.a_max and meta[64 + 62] != 0 and meta[64 + 63] == 0


def test_signature_and_version(hip_lib, host_lib):
    from tetris_amd import _lib
    assert NAME in _lib.SIGNATURES and NAME in _lib.EXPORTS and hasattr(hip_lib.cdll, NAME)
    assert hasattr(host_lib.cdll, "tetris_host_expand_envs")
    assert _lib.ABI_VERSION == 7 == hip_lib.version() == host_lib.version()
    assert "overlap" in hip_lib.error_string(E_OVERLAP)


def test_header_text_matches_the_binding():
    """the declaration of include/tetris_hip.h, argument by argument, against the ctypes signature"""
    from tetris_amd import _lib
    header = open(os.path.join(ROOT, "include", "tetris_hip.h")).read()
    kinds = {ctypes.c_void_p: "pointer", ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t", ctypes.c_uint64: "uint64_t",
             _lib._dp: "pointer"}
    m = re.search(r"\bint %s\(([^;]*)\);" % NAME, header)
    assert m
    declared, names = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        declared.append("pointer" if "*" in arg else arg.rsplit(" ", 1)[0].replace("const ", ""))
        names.append(arg.rsplit(" ", 1)[1].lstrip("*"))
    assert declared == [kinds[t] for t in _lib.SIGNATURES[NAME]]
    assert names == ["desc", "src_cols", "src_meta", "B_src", "dst_cols", "dst_meta", "parent", "action", "next_piece", "obs",
                     "reward", "done", "lines", "n_valid", "piece", "status", "seed", "step_idx", "env_offset", "B_dst",
                     "hip_stream"]
    assert "#define TETRIS_HIP_ABI_VERSION 7" in header
