#!/usr/bin/env python3
"""Generates tetris_amd/csrc/tetris_feature_lut.inc: the byte tables board_features reads from LDS.
Every field has its own uint8 table so the kernels use what they read without shifting or masking
(the kernels are integer-VALU bound, the LDS pipe is not).  Layout (offsets = tet::kLut* in
tetris_core.hpp):

  (written for the 12-row-chunk tables; the 10-row set tetris_feature_lut10.inc is the same with 10 for 12)
  hole_A [8192]  hole_u [8192]      index v = 13 bits: bits 0-11 a 12-row chunk of one column,
      bit 12 the cell just above the chunk.  A hole-run top inside the chunk is a row r <= 11 with
      v[r] = 0 and v[r+1] = 1.  u = number of such rows, A = sum over them of the filled cells of the
      chunk above r (rows r+1..11).  hole_depth(column) (state.py:200,216,239)
      = sum over chunks k of A_k + u_k * popcount(x >> 12(k+1));  column transitions = 2 * sum u_k.

  wells_S [4096]  wells_lead [4096]  wells_trail [4096]    index v = a 12-row chunk of one column's
      well-cell set.  Every maximal run of k cells adds k(k+1)/2 (state.py:228-229,267-268).
      S = sum of the triangles of all runs inside the chunk, lead = length of the run touching row 0
      of the chunk, trail = length of the run touching row 11.  Chunks combine bottom-up:
        total += S + carry * lead;  carry = (lead == 12) ? carry + 12 : trail
      because joining runs of a and b cells adds a*b to the sum of their two triangles.

  sel_pair [256 * 8]   index (a | b << 4) * 8 + k: a, b = the same 4-column group of the two
      orientation fields of one loop of the valid mask.  The reference numbers the placements of a
      loop by column, orientation 0 before 1 (game.py:69 over tetromino.py's loops), i.e. in the
      order a0 b0 a1 b1 a2 b2 a3 b3; entry = (column within the group) | orientation << 2 of the
      k-th set bit in that order (0 where k is past the last one).
  sel_nib [16 * 4]     index nib * 4 + k: position of the k-th set bit of a nibble (bag draw).

tetris_feature_lut10.inc only, after sel_nib (the step kernels' form for 32-bit boards of up to ten columns,
tet::board_features_u32_2x10, which stages sel_pair .. the end and not the byte tables):
  hole_pack [2048 * 2]   (little-endian uint16 entries) index as hole_A / hole_u:  u | A << 8.  Entries are
      ADDED as whole words (sum of u over a board <= 100 stays inside its byte) and split once per board.
  wells_pack [1024 * 4]  (little-endian uint32 entries) index as wells_S:  trail | lead << 8 | S << 16.  Added as
      whole words too (the sums of trail and of lead over two chunks of ten columns are <= 200 each, S on top).

tetris_after_lut.inc (tet::AfterLut, the afterstate kernels): hole_A [8192], hole_u [8192] as above for
12-row chunks, then sel_pair / sel_nib as above after
  wells_pack [4096 * 4]  (little-endian uint32 entries) index v = a 12-row chunk of a column's well-cell
      set: S | trail << 16 | lead << 24 -- the three fields of the byte tables in ONE read per chunk (the
      afterstate walk evaluates the wells of four columns per placement and is bound by the number of LDS
      reads; the stepping kernels, bound by vector instructions, keep the ready-to-use byte tables).
"""
import os

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tetris_amd", "csrc")


def tables(cr):
    """hole_A, hole_u (index: cr rows + the cell above), wells_S, wells_lead, wells_trail (index: cr rows)."""
    hole_a, hole_u = [], []
    for v in range(1 << (cr + 1)):
        A = u = 0
        for r in range(cr):
            if not (v >> r) & 1 and (v >> (r + 1)) & 1:
                u += 1
                A += bin((v & ((1 << cr) - 1)) >> (r + 1)).count("1")
        assert A < 256 and u < 256
        hole_a.append(A)
        hole_u.append(u)
    wells_s, wells_lead, wells_trail = [], [], []
    for v in range(1 << cr):
        S = run = lead = 0
        for r in range(cr):
            if (v >> r) & 1:
                run += 1
            else:
                S += run * (run + 1) // 2
                run = 0
        S += run * (run + 1) // 2
        trail = run
        while lead < cr and (v >> lead) & 1:
            lead += 1
        assert S < 256
        wells_s.append(S)
        wells_lead.append(lead)
        wells_trail.append(trail)
    out = hole_a + hole_u + wells_s + wells_lead + wells_trail + select_tables()
    if cr == 10:  # packed entries for tet::board_features_u32_2x10
        for v in range(1 << (cr + 1)):
            out += [hole_u[v], hole_a[v]]
        for v in range(1 << cr):
            out += [wells_trail[v], wells_lead[v], wells_s[v], 0]
    return out


def select_tables():
    sel_pair = []
    for idx in range(256):
        a, b = idx & 15, idx >> 4
        order = []
        for c in range(4):
            if (a >> c) & 1:
                order.append(c)
            if (b >> c) & 1:
                order.append(c | 4)
        sel_pair += (order + [0] * 8)[:8]
    sel_nib = []
    for nib in range(16):
        pos = [c for c in range(4) if (nib >> c) & 1]
        sel_nib += (pos + [0] * 4)[:4]
    return sel_pair + sel_nib


def after_tables(cr=12):
    t = tables(cr)
    ne, nw = 1 << (cr + 1), 1 << cr
    hole_a, hole_u = t[:ne], t[ne:2 * ne]
    ws, wl, wt = t[2 * ne:2 * ne + nw], t[2 * ne + nw:2 * ne + 2 * nw], t[2 * ne + 2 * nw:2 * ne + 3 * nw]
    out = hole_a + hole_u
    for v in range(nw):
        e = ws[v] | (wt[v] << 16) | (wl[v] << 24)
        out += [e & 255, (e >> 8) & 255, (e >> 16) & 255, (e >> 24) & 255]
    return out + select_tables()  # sel_pair, sel_nib: the step of the in-kernel greedy policies decodes actions too


vals = after_tables(12)
assert len(vals) == 2 * 8192 + 4 * 4096 + 2048 + 64
with open(os.path.join(CSRC, "tetris_after_lut.inc"), "w") as f:
    f.write("// generated by tools/gen_feature_lut.py (afterstate kernels: 12-row chunks, packed wells entries) -- do not edit\n")
    for i in range(0, len(vals), 32):
        f.write(",".join(str(x) for x in vals[i:i + 32]) + ",\n")
print("tetris_after_lut.inc", len(vals))

for cr, name in ((12, "tetris_feature_lut.inc"), (10, "tetris_feature_lut10.inc")):
    vals = tables(cr)
    assert len(vals) == 2 * (1 << (cr + 1)) + 3 * (1 << cr) + 2048 + 64 + (8 * (1 << cr) if cr == 10 else 0) and len(vals) % 16 == 0
    out = os.path.join(CSRC, name)
    with open(out, "w") as f:
        f.write("// generated by tools/gen_feature_lut.py (%d-row chunks) -- do not edit\n" % cr)
        for i in range(0, len(vals), 32):
            f.write(",".join(str(x) for x in vals[i:i + 32]) + ",\n")
    print(out, len(vals), max(vals))
