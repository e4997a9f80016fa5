"""CPU checks of the functions whose bodies the step trim changed, through a g++ build of the lane code
(tests/harness/trim_host.cpp, compiled here into a temporary directory):
  * the table's StampRow against unpack_orient, for the default set, the standard-7 set and all nine pieces;
  * stamp_scratch (clamped and padded form) + clear_lines against the oracle's placements on the directed
    boards: every catalogue piece, orientation and left column, the rightmost ones included (c + j >= C);
  * pack_board / unpack_board against a cell-by-cell restatement written here, on the 24-bit (48-bit) field
    border patterns, C = 5..12 on 32-bit words and 10 columns on 64-bit words."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import directed_boards as db
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
P64 = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("trim") / "libtrim_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(HERE, "harness", "trim_host.cpp"), "-o", so])
    return ctypes.CDLL(so)


def _rows(lib, C, ids):
    out = np.zeros((12, 4, 4), np.uint32)
    a = np.asarray(ids, np.int32)
    assert lib.trim_table_rows(C, len(ids), a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def _orient(lib, desc):
    o = np.zeros(11, np.int32)
    lib.trim_unpack_orient(ctypes.c_uint32(int(desc)), o.ctypes.data_as(ctypes.c_void_p))
    return dict(w=int(o[0]), H=int(o[1]), b=o[2:6].tolist(), n=o[6:10].tolist(), exists=bool(o[10]))


def _set_ids(name):
    return [orc.CATALOGUE.index(n) for n in orc.PIECE_SETS[name]]


@pytest.mark.parametrize("ids", [_set_ids("default"), _set_ids("standard7"), list(range(9))],
                         ids=["default", "standard7", "catalogue"])
def test_stamp_row_against_unpack_orient(lib, ids):
    rows = _rows(lib, 10, ids)
    for i in range(12):
        for k in range(4):
            shape4, bias4, H, desc = (int(x) for x in rows[i, k])
            o = _orient(lib, desc)
            if not (i < len(ids) and o["exists"]):
                assert shape4 == 0 and bias4 == 0x40404040, "a slot without an orientation has no column"
                continue
            assert H == o["H"]
            for j in range(4):
                sj, bj = (shape4 >> (8 * j)) & 255, (bias4 >> (8 * j)) & 255
                if j < o["w"]:
                    assert sj == ((1 << o["n"][j]) - 1) << o["b"][j] and bj == o["b"][j]
                else:
                    assert sj == 0 and bj == 64  # never the minimum: > the leading zeros of any word


def _slots(lib, pid):
    """(slot, width) of the orientations of one catalogue piece that exist"""
    rows = _rows(lib, 10, [pid])
    out = []
    for k in range(4):
        o = _orient(lib, rows[0, k, 3])
        if o["exists"]:
            out.append((k, o["w"]))
    return out


@pytest.mark.parametrize("C,R", [(5, 20), (8, 20), (10, 20), (12, 20), (10, 40)])
def test_stamp_and_clear_against_oracle_on_directed_boards(lib, C, R):
    wb = 4 if R + 4 <= 31 else 8
    boards = np.concatenate([db.structured(R, C, 3), db.near_top(12, R, C, 5)])
    db.check_boards(boards, R)
    desc = orc.make_desc(C, R, orc.CATALOGUE)
    n_right = 0
    for b in boards:
        cols = orc.cells_to_cols(b).astype(np.uint64)
        for pid, name in enumerate(orc.CATALOGUE):
            ref = orc.placements(desc, b, name)
            slots = _slots(lib, pid)
            order = []  # the reference's enumeration: loop, left column, orientation
            for L in (0, 1):
                sl = [(k, w) for k, w in slots if k // 2 == L]
                if sl:
                    for c in range(C - sl[0][1] + 1):
                        order += [(k, c, w) for k, w in sl]
            assert len(order) == len(ref["cells"])
            for row, (k, c, w) in enumerate(order):
                n_right += c + 3 >= C
                for pad in (0, 1):
                    out = np.zeros(C, np.uint64)
                    a, er = ctypes.c_int(0), ctypes.c_int(0)
                    n = lib.trim_stamp_clear(C, wb, pad, pid, k, c, cols.ctypes.data_as(P64), out.ctypes.data_as(P64),
                                             ctypes.byref(a), ctypes.byref(er))
                    what = "%s slot %d column %d pad %d" % (name, k, c, pad)
                    assert n == ref["n_cleared"][row], what
                    assert a.value == ref["anchor_row"][row], what
                    assert np.array_equal(out, orc.cells_to_cols(ref["cells"][row]).astype(np.uint64)), what
    assert n_right > 0


def _plain_pack(cols, C, Wb):
    """cell by cell: bit r of column c is bit c * F + r of one long bit string cut into Wb-bit words"""
    F = Wb * 3 // 4
    s = 0
    for c in range(C):
        for r in range(F):
            if (int(cols[c]) >> r) & 1:
                s |= 1 << (c * F + r)
    n_planes = (C * F + Wb - 1) // Wb
    return [(s >> (Wb * p)) & ((1 << Wb) - 1) for p in range(n_planes)]


def _patterns(C, F, rows):
    full = (1 << rows) - 1
    pats = [[0] * C, [full] * C, [(1 << F) - 1] * C]
    for c in range(C):
        for bit in (0, 7, 8, 15, 16, rows - 1, F - 1):
            p = [0] * C
            p[c] = 1 << bit
            pats.append(p)
            q = [full] * C
            q[c] = full & ~(1 << min(bit, rows - 1))
            pats.append(q)
    rng = np.random.RandomState(C)
    pats += [[int(x) & full for x in rng.randint(0, 1 << 30, C)] for _ in range(8)]
    return pats


@pytest.mark.parametrize("C,wb", [(c, 4) for c in range(5, 13)] + [(10, 8)])
def test_pack_unpack_round_trip_against_plain_restatement(lib, C, wb):
    Wb = 8 * wb
    F = Wb * 3 // 4
    for pat in _patterns(C, F, F):  # every row of the field: all ones below row R + 4 = F at the tallest board
        cols = np.asarray(pat, np.uint64)
        planes, back = np.zeros(12, np.uint64), np.zeros(C, np.uint64)
        npl = lib.trim_pack_unpack(C, wb, cols.ctypes.data_as(P64), planes.ctypes.data_as(P64), back.ctypes.data_as(P64))
        want = _plain_pack(pat, C, Wb)
        assert npl == len(want)
        assert [int(x) for x in planes[:npl]] == want
        assert np.array_equal(back, cols)
