"""CPU-only: tetris_hip_gather_envs refuses bad arguments with the code include/tetris_hip.h names, before any
launch, in the real library (no GPU is needed: it returns first) and in the CPU harness (the same text,
csrc/tetris_abi.inc)."""
import ctypes

import pytest

E_NULL, E_DESC, E_BATCH, E_OVERLAP = -1, -2, -6, -9  # include/tetris_hip.h


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
    """(label, arguments, code).  d: a 10x20 descriptor (8 planes of 4-byte words: 2048 B of cols per tile), z: a
    zeroed one.  The buffers are ADDRESSES nothing may dereference: 64 src envs (cols 2048 B, meta 512 B) and
    100 dst envs (cols 4096 B, meta 800 B), far apart."""
    src_cols, src_meta, dst_cols, dst_meta, other = (base + k * (1 << 20) for k in range(5))
    # desc src_cols src_meta B_src dst_cols dst_meta dst_n_valid dst_piece index status B_dst hip_stream
    good = [d, src_cols, src_meta, 64, dst_cols, dst_meta, None, None, other, None, 100, None]
    rows = []

    def vary(label, at, value, code):
        args = list(good)
        for a, v in zip(at if isinstance(at, tuple) else (at,), value if isinstance(at, tuple) else (value,)):
            args[a] = v
        rows.append((label, args, code))

    for name, at in (("desc", 0), ("src_cols", 1), ("src_meta", 2), ("dst_cols", 4), ("dst_meta", 5), ("index", 8)):
        vary("%s NULL" % name, at, None, E_NULL)
    vary("zeroed descriptor", 0, z, E_DESC)
    for name, at in (("B_src", 3), ("B_dst", 10)):
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
def test_gather_envs_refusals(which, hip_lib, host_lib):
    from tetris_amd import _lib
    lib = hip_lib if which == "hip" else host_lib
    d, z = _lib.TetrisDesc(), _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    assert lib.n_planes(ctypes.byref(d)) == 8 and d.word_bytes == 4
    rows = _rows(ctypes.byref(d), ctypes.byref(z), 1 << 40)
    assert len({r[0] for r in rows}) == len(rows) == 20
    got = [(label, lib.gather_envs(*args), code) for label, args, code in rows]
    assert [g for g in got if g[1] != g[2]] == []


def test_adjacent_storage_is_not_overlap(host_lib):
    """dst right behind src (and right before it) shares no byte: the call gets past every check of the text.
    Harness only (a call that passes its checks runs): it is the same text in the library."""
    from tetris_amd import _lib
    lib = host_lib
    d = _lib.TetrisDesc()
    assert lib.desc_init(ctypes.byref(d), 10, 20, (ctypes.c_int32 * 2)(4, 3), 2, None) == 0
    cols = (ctypes.c_uint32 * (3 * 512))()   # src tile | dst tile | src tile (second call)
    meta = (ctypes.c_uint64 * (3 * 64))()
    index = (ctypes.c_int32 * 64)(*([-1] * 64))
    a, m = ctypes.addressof(cols), ctypes.addressof(meta)
    assert lib.gather_envs(ctypes.byref(d), a, m, 64, a + 2048, m + 512, None, None, ctypes.addressof(index), None, 64, None) == 0
    assert lib.gather_envs(ctypes.byref(d), a + 4096, m + 1024, 64, a + 2048, m + 512, None, None, ctypes.addressof(index), None, 64, None) == 0


@pytest.mark.parametrize("which", ["hip", "host"])
def test_error_string_names_the_overlap(which, hip_lib, host_lib):
    lib = hip_lib if which == "hip" else host_lib
    assert "overlap" in lib.error_string(E_OVERLAP)
    from tetris_amd import _lib
    assert "tetris_hip_gather_envs" in _lib.SIGNATURES and _lib.ABI_VERSION == 7 == lib.version()
