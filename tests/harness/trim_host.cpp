// trim_host.cpp -- g++ build of the per-lane functions whose bodies the step trim changed (stamp through the
// table's StampRow, clear_lines behind it, pack / unpack of the planes), one C entry each, for
// tests/test_step_trim_cpu.py.  Test-only; the product path is the HIP kernels.
#include <stdint.h>
#include <string.h>

#include "../../tetris_amd/csrc/tetris_table.hpp"

namespace {

template <typename W, int C, bool PAD>
int stamp_clear(const uint64_t* in, int c, const tet::StampRow& row, uint64_t* out, int* a_out, int* eroded) {
  W col[C], pbits[4];
  W scratch[C + 3] = {};
  for (int i = 0; i < C; ++i) col[i] = (W)in[i];
  const int a = tet::stamp_scratch<W, C, PAD>(col, scratch, 1, c, row, pbits);
  const int k = tet::clear_lines<W, C>(col, pbits, a, eroded);
  for (int i = 0; i < C; ++i) out[i] = (uint64_t)col[i];
  *a_out = a;
  return k;
}

template <typename W, int C>
void pack_unpack(const uint64_t* in, uint64_t* planes, uint64_t* back) {
  constexpr int NP = tet::n_planes(C, true);
  W col[C], w[NP], col2[C];
  for (int i = 0; i < C; ++i) col[i] = (W)in[i];
  tet::pack_board<W, C, true>(col, w);
  tet::unpack_board<W, C, true>(w, col2);
  for (int p = 0; p < NP; ++p) planes[p] = (uint64_t)w[p];
  for (int i = 0; i < C; ++i) back[i] = (uint64_t)col2[i];
}

}  // namespace

extern "C" {

// rows of the table for a piece list: per (piece, slot) shape4, bias4, H, desc
int trim_table_rows(int C, int n_pieces, const int32_t* piece_ids, uint32_t* out) {
  TetrisDesc d;
  if (tet::desc_init(&d, C, 20, piece_ids, n_pieces, nullptr) != TETRIS_OK) return -1;
  tet::SetTable t;
  tet::build_table(&d, &t);
  for (int i = 0; i < tet::kMaxPieces; ++i)
    for (int k = 0; k < 4; ++k) {
      uint32_t* o = out + (i * 4 + k) * 4;
      o[0] = t.stamp[i][k].shape4;
      o[1] = t.stamp[i][k].bias4;
      o[2] = t.stamp[i][k].H;
      o[3] = t.orient[i][k].desc;
    }
  return 0;
}

// unpack_orient of a descriptor: w, H, b[4], n[4], exists
void trim_unpack_orient(uint32_t desc, int32_t* out) {
  const tet::Orient o = tet::unpack_orient(desc);
  out[0] = o.w;
  out[1] = o.H;
  for (int j = 0; j < 4; ++j) {
    out[2 + j] = o.b[j];
    out[6 + j] = o.n[j];
  }
  out[10] = o.exists ? 1 : 0;
}

// stamp slot `sk` of catalogue piece `pid` at left column c, then clear; returns lines cleared (-1: bad geometry)
int trim_stamp_clear(int C, int word_bytes, int pad, int pid, int sk, int c, const uint64_t* in, uint64_t* out, int* a_out,
                     int* eroded) {
  TetrisDesc d;
  const int32_t ids[1] = {pid};
  if (tet::desc_init(&d, C, word_bytes == 4 ? 20 : 40, ids, 1, nullptr) != TETRIS_OK) return -1;
  tet::SetTable t;
  tet::build_table(&d, &t);
  const tet::StampRow& row = t.stamp[0][sk];
#define TET_X(CC)                                                                                                      \
  if (C == CC && word_bytes == 4) return pad ? stamp_clear<uint32_t, CC, true>(in, c, row, out, a_out, eroded)         \
                                             : stamp_clear<uint32_t, CC, false>(in, c, row, out, a_out, eroded);       \
  if (C == CC && word_bytes == 8) return pad ? stamp_clear<uint64_t, CC, true>(in, c, row, out, a_out, eroded)         \
                                             : stamp_clear<uint64_t, CC, false>(in, c, row, out, a_out, eroded);
  TET_COLUMNS(TET_X)
#undef TET_X
  return -1;
}

int trim_pack_unpack(int C, int word_bytes, const uint64_t* in, uint64_t* planes, uint64_t* back) {
#define TET_X(CC)                                                                            \
  if (C == CC && word_bytes == 4) { pack_unpack<uint32_t, CC>(in, planes, back); return tet::n_planes(CC, true); } \
  if (C == CC && word_bytes == 8) { pack_unpack<uint64_t, CC>(in, planes, back); return tet::n_planes(CC, true); }
  TET_COLUMNS(TET_X)
#undef TET_X
  return -1;
}

}  // extern "C"
