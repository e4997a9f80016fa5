// lane_equivalence.cpp -- TEST HARNESS ONLY (tests/test_step_lane_equivalence.py compiles it with g++).
// Compares tet::valid_mask (the top-rows form env_step uses on 32-bit boards AND the general form refresh_kernel
// keeps) and tet::board_features (12-row tables, and the packed 10-row form where R <= 20) with ONE yardstick
// that is no form of them: plain loops over a board's cells, no tables and no bit-parallel words.  The valid
// mask is worked out one placement at a time by the rule stated above valid_mask in tetris_core.hpp, the six
// feature integers cell by cell as oracle/tetris_oracle.c states them.  The yardstick takes only the piece
// geometry (tet::kCatalogue) and the mask layout (tet::mask_bit) from the product, and the test pins it to the
// oracle: its masks to the terminal flags of the oracle's placements, its features to the oracle's.
#include <stdint.h>
#include <string.h>

#include "../../include/tetris_hip.h"
#include "../../tetris_amd/csrc/tetris_core.hpp"
#include "../../tetris_amd/csrc/tetris_table.hpp"

namespace {

typedef uint32_t W;
constexpr int kMaxStoredRows = 32;  // R + 4 stored rows of a 32-bit board

// ======================= the yardstick: cells, loops, no tables ===========================================
// A board as the yardstick sees it, with its walls: columns -1 and C, filled on every stored row.  The boards
// it is given hold no cell at or above row R (the callers count the others as dirty and leave them out).
template <int C>
struct Cells {
  int8_t cell[kMaxStoredRows][C + 2];  // cell[r][c + 1] = cell (r, c), row 0 = bottom; [0] and [C + 1] the walls
  int h[C];                            // lowest free row of each column
  int filled[kMaxStoredRows];          // cells in each row, walls left out
};

template <int C>
void cells_of(const W (&col)[C], int R, Cells<C>* b) {
  for (int r = 0; r < R + 4; ++r) {
    b->cell[r][0] = b->cell[r][C + 1] = 1;
    b->filled[r] = 0;
    for (int c = 0; c < C; ++c) {
      b->cell[r][c + 1] = (int8_t)((col[c] >> r) & 1u);
      b->filled[r] += b->cell[r][c + 1];
    }
  }
  for (int c = 0; c < C; ++c) {
    b->h[c] = R + 4;
    while (b->h[c] > 0 && !b->cell[b->h[c] - 1][c + 1]) --b->h[c];
  }
}

// What a placement needs of one orientation: its width, its height H = max_j (b_j + n_j), the bottom offsets
// b_j of its columns and the number of its cells in each of its rows.  Read once from the catalogue.
struct Shape {
  int w, H, b[4], in_row[4];
};
struct Shapes {
  Shape of[TETRIS_N_CATALOGUE][4];  // [piece][k = 2L + o]; w = 0: no such orientation
  Shapes() {
    memset(of, 0, sizeof(of));
    for (int p = 0; p < TETRIS_N_CATALOGUE; ++p)
      for (int l = 0; l < 2; ++l)
        for (int oi = 0; oi < tet::kCatalogue[p].n_orient[l]; ++oi) {
          const tet::CatOrient& o = tet::kCatalogue[p].o[l][oi];
          Shape& s = of[p][2 * l + oi];
          s.w = o.w;
          for (int j = 0; j < o.w; ++j) {
            s.b[j] = o.b[j];
            if (o.b[j] + o.n[j] > s.H) s.H = o.b[j] + o.n[j];
            for (int k = o.b[j]; k < o.b[j] + o.n[j]; ++k) ++s.in_row[k];
          }
        }
  }
};
const Shapes kShapes;

// One placement: shape s with its left column at c.  The piece lands at a = max_j (h[c+j] - b_j), so its cells
// fall on free cells; the rows a .. a+H-1 that are full with them are removed and the rows above drop; the
// placement is terminal iff a cell remains at row >= R.  The stack holds no cell there and rows only move down,
// so only the piece's own rows can: each is visited bottom up with the number of rows removed below it.
// *rescued: the piece poked above row R - 1 before the clear and the placement is not terminal after it.
template <int C>
inline bool placement_survives(const Cells<C>& b, const Shape& s, int c, int R, bool* rescued) {
  int a = 0;
  for (int j = 0; j < s.w; ++j)
    if (b.h[c + j] - s.b[j] > a) a = b.h[c + j] - s.b[j];
  int removed = 0;
  bool terminal = false;
  for (int k = 0; k < s.H; ++k) {
    const bool full = b.filled[a + k] + s.in_row[k] == C;
    removed += full;
    terminal |= !full & (a + k - removed >= R);  // a row of the piece that stays: it holds a cell
  }
  *rescued = a + s.H > R && !terminal;
  return !terminal;
}

// bit mask_bit(2L + o, c) is set iff the placement exists (the orientation does, and c + w <= C) and is not terminal
template <int C>
uint64_t yardstick_mask(const Cells<C>& b, int piece, int R, int64_t* n_rescued) {
  uint64_t mask = 0;
  for (int k = 0; k < 4; ++k) {
    const Shape& s = kShapes.of[piece][k];
    if (s.w == 0) continue;
    for (int c = 0; c + s.w <= C; ++c) {
      bool rescued;
      mask |= (uint64_t)placement_survives<C>(b, s, c, R, &rescued) << tet::mask_bit(k, c);
      *n_rescued += rescued;
    }
  }
  return mask;
}

// The six feature integers, cell by cell, as oracle/tetris_oracle.c states them (rows with holes, column
// transitions, holes, cumulative wells, row transitions, hole depth).  The walls are R high.
//  * a hole is a free cell below its column's top; its depth counts, when the cell on top of it is filled, the
//    filled cells of the column above it;
//  * column transitions: changes of filled / free along a column from the floor (filled) to its top, and one
//    more for the free cell above the top (an empty column has that one alone);
//  * row transitions: below a column's top, every cell that differs from its left neighbour, and the rows by
//    which the left neighbour is higher; an empty column counts its left neighbour's filled cells instead; the
//    right wall counts R less the filled cells of the last column;
//  * a well cell is a free cell with both neighbours filled, below the column's top or, above it, below the
//    lower of the neighbours' tops; every well cell adds the length of the unbroken run of well cells that ends
//    in it (a run of n adds n(n+1)/2).
template <int C>
void yardstick_features(const Cells<C>& b, int R, int (&f)[6]) {
  auto at = [&](int r, int c) { return (int)b.cell[r][c + 1]; };
  auto top = [&](int c) { return (c < 0 || c >= C) ? R : b.h[c]; };
  bool row_has_hole[kMaxStoredRows] = {false};
  int col_trans = 0, holes = 0, wells = 0, row_trans = 0, hole_depth = 0;
  for (int c = 0; c < C; ++c) {
    const int h = top(c), hl = top(c - 1), hr = top(c + 1);
    int above = 0;  // filled cells of the column above the row in hand
    for (int r = 0; r < h; ++r) above += at(r, c);
    int run = 0;    // well cells in an unbroken run up to the row in hand
    col_trans += 1;
    for (int r = 0; r < h; ++r) {  // (sums of 0 / 1 terms: the cells are random, branches on them cost more)
      const int cell = at(r, c), hole = 1 - cell;
      const int well = hole & at(r, c - 1) & at(r, c + 1);
      col_trans += cell != (r > 0 ? at(r - 1, c) : 1);
      row_trans += cell != at(r, c - 1);
      above -= cell;
      holes += hole;
      row_has_hole[r] |= (bool)hole;
      hole_depth += hole * at(r + 1, c) * above;
      run = well * (run + 1);
      wells += run;
    }
    if (h > 0)
      row_trans += hl > h ? hl - h : 0;
    else
      for (int r = 0; r < hl; ++r) row_trans += at(r, c - 1);
    for (int r = h; r < hl && r < hr; ++r) {
      run = (at(r, c - 1) & at(r, c + 1)) * (run + 1);
      wells += run;
    }
  }
  row_trans += R;
  for (int r = 0; r < R + 4; ++r) row_trans -= at(r, C - 1);
  f[0] = 0;
  for (int r = 0; r < R + 4; ++r) f[0] += row_has_hole[r];
  f[1] = col_trans;
  f[2] = holes;
  f[3] = wells;
  f[4] = row_trans;
  f[5] = hole_depth;
}
// ======================= end of the yardstick =============================================================

struct alignas(16) Lut12 { uint8_t bytes[tet::kFeatureLutBytes]; };
const Lut12 kLut12 = {{
#include "../../tetris_amd/csrc/tetris_feature_lut.inc"
}};
struct alignas(16) Lut10 { uint8_t bytes[tet::kFeatureLut10Bytes]; };
const Lut10 kLut10 = {{
#include "../../tetris_amd/csrc/tetris_feature_lut10.inc"
}};

void make_table(int C, int n_pieces, const int32_t* piece_ids, tet::SetTable* t) {
  TetrisDesc d;
  memset(&d, 0, sizeof(d));
  d.num_columns = C;
  d.n_pieces = n_pieces;
  for (int i = 0; i < n_pieces; ++i) d.piece_ids[i] = piece_ids[i];
  tet::build_table(&d, t);
}

struct Tally {
  int64_t mask_bad = 0, feat_bad = 0, masks = 0;
  int64_t rescued[16] = {0};
  void add(const Tally& o) {
    mask_bad += o.mask_bad;
    feat_bad += o.feat_bad;
    masks += o.masks;
    for (int i = 0; i < 16; ++i) rescued[i] += o.rescued[i];
  }
};
#pragma omp declare reduction(+ : Tally : omp_out.add(omp_in))

// One clean board: valid_mask of every piece of the set in both present forms, and board_features in the table
// variants the kernels instantiate for R, against the yardstick.
template <int C>
void check_board(const W (&col)[C], const Cells<C>& b, int R, const tet::SetTable& tab, int n_pieces,
                 const int32_t* piece_ids, Tally* t) {
  int h[C];
  tet::heights_of<W, C>(col, h);
  for (int i = 0; i < n_pieces; ++i) {
    const uint64_t want = yardstick_mask<C>(b, piece_ids[i], R, &t->rescued[i]);
    t->mask_bad += tet::valid_mask<W, C, true>(col, h, tab.orient[i], tab.fullmask[i], R) != want;
    t->mask_bad += tet::valid_mask<W, C, false>(col, h, tab.orient[i], tab.fullmask[i], R) != want;
    ++t->masks;
  }
  int f[6], g[6];
  yardstick_features<C>(b, R, g);
  tet::board_features<W, C, 0, 12>(col, h, R, kLut12.bytes, f[0], f[1], f[2], f[3], f[4], f[5]);
  t->feat_bad += memcmp(f, g, sizeof(f)) != 0;
  if (R <= 20) {  // the 10-row-chunk tables of the stepping kernels (board_features_u32_2x10)
    tet::board_features<W, C, 2, 10>(col, h, R, kLut10.bytes, f[0], f[1], f[2], f[3], f[4], f[5]);
    t->feat_bad += memcmp(f, g, sizeof(f)) != 0;
  }
}

inline uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Set (i): rows R-4 .. R-1 of a 6-column window run through patterns (every `every`-th of the 2^24, offset by a
// hash so that no bit is fixed), the window at every position 0 .. C-6; the other columns' top rows and every
// row below R-4 are random (fixed seed); no cell at or above R.
inline uint32_t window_pattern(uint64_t seed, int every, int64_t q) {
  return (uint32_t)(q * every + (int64_t)(mix64(seed ^ (uint64_t)q) % (uint64_t)every));
}

template <int C>
void window_board(int R, uint64_t seed, uint32_t pat, int pos, W (&col)[C]) {
  const uint64_t r0 = mix64(seed * 31 + (uint64_t)pat * 8 + (uint64_t)pos);
  for (int c = 0; c < C; ++c) {
    const uint64_t rc = mix64(r0 + (uint64_t)c);
    // below R-4: random cells, thinned or thickened by a per-column choice so that rows are sometimes near full
    W low = (W)rc;
    if ((rc >> 40) & 1) low |= (W)(rc >> 8);
    if ((rc >> 41) & 1) low |= (W)(rc >> 16);
    low &= tet::lowmask<W>(R - 4);
    W top = (c >= pos && c < pos + 6) ? (W)((pat >> (4 * (c - pos))) & 15u) : (W)((rc >> 44) & 15u);
    if (!(c >= pos && c < pos + 6) && ((rc >> 48) & 3) != 0) top = 15u >> ((rc >> 50) & 1);  // mostly stacked: rescues need it
    col[c] = (W)(low | (top << (R - 4)));
  }
}

template <int C>
int64_t window_run(int R, int n_pieces, const int32_t* piece_ids, uint64_t seed, int every, int64_t* rescued,
                   int64_t* checked, int64_t* feat_bad) {
  tet::SetTable tab;
  make_table(C, n_pieces, piece_ids, &tab);
  Tally t;
  const int64_t n_pat = ((int64_t)1 << 24) / every;
#pragma omp parallel for schedule(static) reduction(+ : t)
  for (int64_t q = 0; q < n_pat; ++q) {
    const uint32_t pat = window_pattern(seed, every, q);
    for (int pos = 0; pos + 6 <= C; ++pos) {
      W col[C];
      Cells<C> b;
      window_board<C>(R, seed, pat, pos, col);
      cells_of<C>(col, R, &b);
      check_board<C>(col, b, R, tab, n_pieces, piece_ids, &t);
    }
  }
  for (int i = 0; i < n_pieces; ++i) rescued[i] += t.rescued[i];
  *checked += t.masks;
  *feat_bad += t.feat_bad;
  return t.mask_bad;
}

}  // namespace

extern "C" {

// Set (i) on C = 8 or 10 columns, every piece of the set.  Returns the number of mask mismatches (-1: C not built);
// rescued[i] += rescued placements seen for piece i; *checked += masks compared; *feat_bad += feature mismatches.
int64_t lane_vm_window(int C, int R, int n_pieces, const int32_t* piece_ids, uint64_t seed, int every,
                       int64_t* rescued, int64_t* checked, int64_t* feat_bad) {
  if (C == 8) return window_run<8>(R, n_pieces, piece_ids, seed, every, rescued, checked, feat_bad);
  if (C == 10) return window_run<10>(R, n_pieces, piece_ids, seed, every, rescued, checked, feat_bad);
  return -1;
}

// The boards of set (i) themselves (ten columns): cols[(q * 5 + pos) * 10 + c], (2^24 / every) * 5 boards.
void lane_window_cols(int R, uint64_t seed, int every, uint32_t* cols) {
  const int64_t n_pat = ((int64_t)1 << 24) / every;
  for (int64_t q = 0; q < n_pat; ++q)
    for (int pos = 0; pos < 5; ++pos) {
      W col[10];
      window_board<10>(R, seed, window_pattern(seed, every, q), pos, col);
      memcpy(cols + (q * 5 + pos) * 10, col, sizeof(col));
    }
}

// Sets (ii), (iii): given boards (ten column words each).  out[0] += mask mismatches, out[1] += feature
// mismatches, out[2] += boards with a cell at or above R (the caller asserts 0), out[3] += masks compared,
// out[4] += wavefronts (64 consecutive boards) whose rescue evaluation runs, out[5] += wavefronts.
void lane_boards(int R, int n_pieces, const int32_t* piece_ids, const uint32_t* cols, int64_t n, int64_t* out) {
  constexpr int C = 10;
  tet::SetTable tab;
  make_table(C, n_pieces, piece_ids, &tab);
  Tally t;
  int64_t dirty = 0, wav_run = 0, wav = 0;
#pragma omp parallel for schedule(static) reduction(+ : t, dirty, wav_run, wav)
  for (int64_t w0 = 0; w0 < n; w0 += 64) {
    bool any = false;
    for (int64_t i = w0; i < w0 + 64 && i < n; ++i) {
      W col[C];
      Cells<C> b;
      bool over = false;
      for (int c = 0; c < C; ++c) {
        col[c] = cols[i * C + c];
        over |= (col[c] >> R) != 0;
      }
      if (over) {
        ++dirty;
        continue;
      }
      cells_of<C>(col, R, &b);
      int n3 = 0;
      for (int c = 0; c < C; ++c) n3 += b.h[c] >= R - 2;
      any |= n3 >= C - 4;
      check_board<C>(col, b, R, tab, n_pieces, piece_ids, &t);
    }
    ++wav;
    wav_run += any;
  }
  out[0] += t.mask_bad;
  out[1] += t.feat_bad;
  out[2] += dirty;
  out[3] += t.masks;
  out[4] += wav_run;
  out[5] += wav;
}

// The yardstick alone, for the test that pins it to the oracle, on clean boards (ten column words each):
// masks[i] = its valid mask of catalogue piece `pid` on board i.
void lane_yardstick_masks(int R, int pid, const uint32_t* cols, int64_t n, uint64_t* masks) {
  constexpr int C = 10;
  for (int64_t i = 0; i < n; ++i) {
    W col[C];
    Cells<C> b;
    int64_t rescued = 0;
    memcpy(col, cols + i * C, sizeof(col));
    cells_of<C>(col, R, &b);
    masks[i] = yardstick_mask<C>(b, pid, R, &rescued);
  }
}

// feats[6 i ..] = its six feature integers of board i
void lane_yardstick_features(int R, const uint32_t* cols, int64_t n, int32_t* feats) {
  constexpr int C = 10;
  for (int64_t i = 0; i < n; ++i) {
    W col[C];
    Cells<C> b;
    int f[6];
    memcpy(col, cols + i * C, sizeof(col));
    cells_of<C>(col, R, &b);
    yardstick_features<C>(b, R, f);
    for (int q = 0; q < 6; ++q) feats[6 * i + q] = f[q];
  }
}

}  // extern "C"
