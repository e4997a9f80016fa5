// lane_parent_equivalence.cpp -- TEST HARNESS ONLY (tests/test_step_lane_parent_equivalence.py compiles it with g++).
// Holds a FROZEN copy of valid_mask (general and top-rows form) and board_features (with col_own, col_rowtrans,
// col_wells) as they stood before the second round of instruction-count work on the step kernel -- the commit
// "valid-mask level sets from the top four rows" -- renamed *_parent, and compares them with the present
// tet::valid_mask and tet::board_features for <uint32_t, 10>.  The copies read the present tables (the fields they
// use did not change) and are never edited along with the product: they are the yardstick.
#include <stdint.h>
#include <string.h>

#include "../../include/tetris_hip.h"
#include "../../tetris_amd/csrc/tetris_core.hpp"
#include "../../tetris_amd/csrc/tetris_table.hpp"

namespace tet {
// ======================= frozen copies of the parent's forms ==============================================
template <typename W, int NCH = 0, int CR = 12>
TET_HD void col_own_parent(W x, int hi, int R, const uint8_t* lut, W& ho, int& nh, int& f1, int& f7) {
  ho = (W)(~x & lowmask<W>(hi));                   // holes (state.py:210-213)
  nh = popc(ho);
  const uint8_t* lut_a = lut + LutLayout<CR>::kHoleA;
  const uint8_t* lut_u = lut + LutLayout<CR>::kHoleU;
  int d7 = 0, u = 0;
  if (!(TET_ABLATE & 16)) {
#pragma unroll
    for (int k = 0; CR * k < (int)(8 * sizeof(W)) - 1; ++k) {
      // rows beyond the stored ones are zero: entry 0 adds nothing, so extra chunks are harmless
      if (NCH > 0 ? k < NCH : (k < 2 || CR * k < R + 4)) {
        const uint32_t up = (uint32_t)(x >> (CR * k));
        const uint32_t idx = (NCH > 0 && k == NCH - 1) ? up : (up & (uint32_t)(LutLayout<CR>::kHoleEntries - 1));
        const int uk = lut_u[idx];
        u += uk;
        d7 += lut_a[idx];
        const bool more = NCH > 0 ? k + 1 < NCH : (CR * (k + 1) < R + 4);  // rows above this chunk exist
        if (CR * (k + 1) < (int)(8 * sizeof(W)) && more) d7 += uk * popc((W)(x >> (CR * (k + 1))));
      }
    }
  }
  f1 = 2 * u;
  f7 = d7;
}

// Row transitions of one column against its LEFT neighbour (state.py:203-204,223-226,
// 246-248,253-254).  Empty column: the filled cells of the left neighbour = hL - its holes
// (:254); otherwise max(hL-h, 0).
template <typename W>
TET_HD int col_rowtrans_parent(W x, W L, int hi, int hL, int nh_left) {
  const int dl = hL - hi;
  return popc((W)((x ^ L) & lowmask<W>(hi))) + (dl > 0 ? dl : 0) - ((hi == 0) ? nh_left : 0);
}

// Cumulative wells of one column (state.py:223-233 inside the column, :258-272 above it).
// A well cell is an empty cell whose two neighbours are filled: inside the column (rows < h) the
// walls count as filled on every stored row (state.py:177-178); above it only rows below
// min(hL, hR) count, with wall height R (state.py:179,258-261) -- neighbours have no cells at or
// above their own height, so for inner columns the set is simply ~x & L & R, and for the edge
// columns the wall side is cut at max(h, R).  Every maximal vertical run of k well cells adds
// k(k+1)/2: summed per 12-row chunk through the wells tables (S, lead, trail) with a carry for
// runs that cross chunk borders -- no data-dependent loop.  (A full chunk has trail = lead = 12.)
template <typename W, int NCH = 0, int CR = 12>
TET_HD int col_wells_parent(W x, W L, W Rr, int hi, int R, bool left_wall, bool right_wall, const uint8_t* lut) {
  W w = (W)(~x & L & Rr);
  if (left_wall || right_wall) w = (W)(w & lowmask<W>(hi > R ? hi : R));
  const uint8_t* lut_s = lut + LutLayout<CR>::kWellsS;
  const uint8_t* lut_lead = lut + LutLayout<CR>::kWellsLead;
  const uint8_t* lut_trail = lut + LutLayout<CR>::kWellsTrail;
  int total = 0, carry = 0;
#pragma unroll
  for (int k = 0; CR * k < (int)(8 * sizeof(W)) - 1; ++k) {
    if (NCH > 0 ? k < NCH : (k < 2 || CR * k < R + 4)) {  // rows beyond the stored ones hold no well cells
      const uint32_t up = (uint32_t)(w >> (CR * k));
      const uint32_t idx = (NCH > 0 && k == NCH - 1) ? up : (up & (uint32_t)(LutLayout<CR>::kWellsEntries - 1));
      const bool last = NCH > 0 && k == NCH - 1;
      total += lut_s[idx];
      if (k == 0) {
        if (!last) carry = lut_trail[idx];
      } else {
        const int lead = lut_lead[idx];
        total += carry * lead;
        if (!last) {
          const int trail = lut_trail[idx];  // read unconditionally: a select, not a branch around the load
          carry = (lead == CR) ? carry + CR : trail;
        }
      }
    }
  }
  return (TET_ABLATE & 32) ? 0 : total;
}

// state.py:175-280.  out = f0,f1,f2,f4,f5,f7.
// PACKW: hole_lut is an AfterLut (packed wells entries) instead of a LutLayout<CR>
template <typename W, int C, int NCH = 0, int CR = 12, bool PACKW = false>
TET_HD void board_features_parent(const W (&col)[C], const int (&h)[C], int R, const uint8_t* hole_lut,
                           int& rows_with_holes, int& col_trans, int& holes, int& wells, int& row_trans,
                           int& hole_depth) {
  const W wall = lowmask<W>(R + 4);  // walls of ones over every stored row (state.py:177-178)
  W hole_rows = 0;
  int f1 = C;                      // one unconditional transition per column (state.py:194)
  int f2 = 0, f4 = 0, f7 = 0;
  int f5 = R - popc(col[C - 1]);   // state.py:190
  int nh_left = 0;                 // holes of the left neighbour (the wall has none)
#pragma unroll
  for (int i = 0; i < C; ++i) {
    const W L = (i == 0) ? wall : col[i - 1];
    const W Rr = (i == C - 1) ? wall : col[i + 1];
    const int hL = (i == 0) ? R : h[i - 1];       // state.py:179 wall height = num_rows
    W ho;
    int nh, d1, d7;
    col_own_parent<W, NCH, CR>(col[i], h[i], R, hole_lut, ho, nh, d1, d7);
    f1 += d1;
    f2 += nh;
    f7 += d7;
    hole_rows |= ho;                              // state.py:215
    f5 += col_rowtrans_parent<W>(col[i], L, h[i], hL, nh_left);
    nh_left = nh;
    if (PACKW)
      f4 += col_wells_packed<W, NCH>(col[i], L, Rr, h[i], R, i == 0, i == C - 1,
                                     reinterpret_cast<const uint32_t*>(hole_lut + AfterLut::kWellsPack));
    else
      f4 += col_wells_parent<W, NCH, CR>(col[i], L, Rr, h[i], R, i == 0, i == C - 1, hole_lut);
    if (TET_FENCE_EVERY > 0 && i % TET_FENCE_EVERY == TET_FENCE_EVERY - 1 && i + 1 < C) {
      TET_PIN(f1);
      TET_PIN(f2);
      TET_PIN(f4);
      TET_PIN(f5);
      TET_PIN(f7);
      TET_SCHED_FENCE();
    }
  }
  rows_with_holes = popc(hole_rows);  // state.py:274-275
  col_trans = f1;
  holes = f2;
  wells = f4;
  row_trans = f5;
  hole_depth = f7;
}

template <typename W, int C, bool TOP = false>
TET_HD uint64_t valid_mask_parent(const W (&col)[C], const int (&h)[C], const OrientEntry* tab, uint64_t fullmask, int R) {
  static_assert(C <= 12, "16-bit level fields; 12-bit mask fields");
  static_assert(!TOP || (sizeof(W) == 4 && C <= 10), "the top-rows form is written for 32-bit boards of up to ten columns");
  constexpr int LS = kLevelStride;
  typedef typename MissBits<C>::type FT;
  const uint32_t cm = (1u << C) - 1u;
  uint32_t zlo, zhi;   // the level word
  uint32_t b3;         // level set 3 (for the rescue test)
  uint32_t mrow[3] = {0u, 0u, 0u};  // TOP: missing cells of rows R-3, R-2, R-1, bit c = column c
  if constexpr (TOP) {
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int g = 0; g < 4 && g < C; ++g) {
      uint32_t pk = (uint32_t)(col[g] >> (R - 4));
      uint32_t sel = 1u;
      if (g + 4 < C) { pk |= (uint32_t)(col[g + 4] >> (R - 4)) << 4; sel |= 1u << 4; }
      if (g + 8 < C) { pk |= (uint32_t)(col[g + 8] >> (R - 4)) << 8; sel |= 1u << 8; }
      const uint32_t u = pk * (0x8001u << g);          // pk << g  |  pk << (15 + g): disjoint, no carries
      const uint32_t mk = (sel * 0x10001u) << g;
      lo |= u & mk;                                    // rows R-4 | R-3 << 16
      hi |= (u >> 2) & mk;                             // rows R-2 | R-1 << 16
    }
    zhi = hi | (hi >> 16);                             // B_2 | B_1 << 16
    zlo = lo | (lo >> 16) | ((zhi & 0xFFFFu) * 0x10001u);  // B_4 | B_3 << 16
    b3 = zlo >> 16;
    mrow[0] = ~(lo >> 16) & cm;
    mrow[1] = ~hi & cm;
    mrow[2] = ~(hi >> 16) & cm;
  } else {
    uint32_t P[3] = {0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < C; ++c) P[c >> 2] |= (uint32_t)h[c] << (8 * (c & 3));
    uint32_t lv[4];
#pragma unroll
    for (int l = 1; l <= 4; ++l) {
      // byte b of P + K has bit 7 set iff h_b > R - l  (h <= 63, K <= 127: no carry between bytes)
      const uint32_t K = (uint32_t)(127 - (R - l)) * 0x01010101u;
      uint32_t g = 0;
#pragma unroll
      for (int q = 0; q < (C + 3) / 4; ++q)
        g |= ((((P[q] + K) & 0x80808080u) * 0x00204081u) >> 28) << (4 * q);  // gather the four bit-7s
      lv[l - 1] = g;
    }
    zlo = lv[3] | (lv[2] << LS);
    zhi = lv[1] | (lv[0] << LS);
    b3 = lv[2];
  }
  const uint64_t Z = ((uint64_t)zhi << 32) | zlo;
  // A placement that pokes above row R - 1 is rescued only by a row among R-3 .. R-1 that the piece
  // completes, i.e. one that misses at most four cells.  A cell in row R-3 or above means h >= R - 2
  // (level set 3), so when fewer than C - 4 columns reach that height no such row exists: the whole
  // rescue evaluation (a third of this function) is skipped -- by the wavefront, when none of its
  // envs needs it, which is the rule for boards that are not stacked to the top.
  const bool rescue = !TET_RESCUE_SKIP || TET_WAVE_ANY(popc(b3) >= C - 4);
  uint32_t X[3] = {0u, 0u, 0u}, Y[3] = {0u, 0u, 0u};
  uint32_t rv1 = 0, rv2 = 0;
  if (rescue) {
    if constexpr (TOP) {
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const uint32_t m = mrow[t];                                      // bit c: column c misses row R-3+t
        const int lo = __builtin_ctz(m | 0x80000000u);
        const int hi = bitlen((uint32_t)(m | 1u)) - 1;
        X[t] = ~0u << hi;
        Y[t] = m ? (2u << lo) - 1u : 0u;  // a full row (only on boards that were set from outside) rescues nothing
      }
    } else {
      FT Fall = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) Fall |= (FT)((uint32_t)(col[c] >> (R - 3)) & 7u) << (3 * c);  // cells of rows R-3..R-1
      const FT Mall = (FT)~Fall;  // missing cells, 3 bits per column
      constexpr FT kEveryThird = (FT)0x9249249249249249ull & (FT)(((FT)1 << (3 * C)) - 1);  // bit 3c
      constexpr FT kTop = (FT)1 << (8 * sizeof(FT) - 1);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const FT m = (FT)(Mall >> t) & kEveryThird;                     // bit 3c: column c misses row R-3+t
        const int lo = (ctz_any((FT)(m | kTop)) * 11) >> 5;              // / 3
        const int hi = ((bitlen((FT)(m | 1)) - 1) * 11) >> 5;            // (bitlen: the top bit of m is never set)
        X[t] = ~0u << hi;
        Y[t] = m ? (2u << lo) - 1u : 0u;  // a full row (only on boards that were set from outside) rescues nothing
      }
    }
    const uint32_t s0 = X[0] & Y[0], s1 = X[1] & Y[1], s2 = X[2] & Y[2];
    rv1 = s0 | s1 | s2;  // vertical Straight: any of its three lower rows
    rv2 = s1 & s2;       //                    / both of R-2, R-1
  }
  uint64_t mask = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const OrientEntry& e = tab[k];
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) r |= (uint32_t)(Z >> e.sh[j]);
    const uint32_t i1 = r, i2 = r >> LS;
    uint32_t v = ~i1;
    if (rescue) {
      // rescue by one cleared row (e = 1)
      uint32_t r1 = ((X[1] >> e.rj1[0]) & (Y[1] >> e.rj0[0])) | ((X[2] >> e.rj1[1]) & (Y[2] >> e.rj0[1]));
      r1 = (rv1 & e.vert4) | (r1 & ~e.vert4);
      const uint32_t r2 = rv2 & e.vert4;
      v |= ~(i2 & ~r2) & r1;
    }
    mask |= (uint64_t)(v & cm) << (kFieldStride * k);
  }
  return mask & fullmask;
}

// ======================= end of the frozen copies =========================================================
}  // namespace tet

namespace {

constexpr int C = 10;
typedef uint32_t W;

struct alignas(16) Lut12 { uint8_t bytes[tet::kFeatureLutBytes]; };
const Lut12 kLut12 = {{
#include "../../tetris_amd/csrc/tetris_feature_lut.inc"
}};
struct alignas(16) Lut10 { uint8_t bytes[tet::kFeatureLut10Bytes]; };
const Lut10 kLut10 = {{
#include "../../tetris_amd/csrc/tetris_feature_lut10.inc"
}};

struct Tables {
  tet::SetTable now;
  int n_pieces;
};

void make_tables(int n_pieces, const int32_t* piece_ids, Tables* t) {
  TetrisDesc d;
  memset(&d, 0, sizeof(d));
  d.num_columns = C;
  d.n_pieces = n_pieces;
  for (int i = 0; i < n_pieces; ++i) d.piece_ids[i] = piece_ids[i];
  tet::build_table(&d, &t->now);
  t->n_pieces = n_pieces;
}

inline uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// valid placements of `mask` whose piece pokes above row R - 1 before the clear (they are valid only through
// the rescue by a cleared row): anchor a = max_j (h[c+j] - b_j), a + H > R.  Independent of both forms.
int count_rescued(uint64_t mask, const tet::CatPiece& p, const int (&h)[C], int R) {
  int n = 0;
  for (int l = 0; l < 2; ++l)
    for (int oi = 0; oi < p.n_orient[l]; ++oi) {
      const tet::CatOrient& o = p.o[l][oi];
      int H = 0;
      for (int j = 0; j < o.w; ++j)
        if (o.b[j] + o.n[j] > H) H = o.b[j] + o.n[j];
      for (int c = 0; c + o.w <= C; ++c) {
        if (!((mask >> tet::mask_bit(2 * l + oi, c)) & 1)) continue;
        int a = 0;
        for (int j = 0; j < o.w; ++j)
          if (h[c + j] - o.b[j] > a) a = h[c + j] - o.b[j];
        if (a + H > R) ++n;
      }
    }
  return n;
}

// board_features in the table variants the kernels instantiate for R, present against parent: 1 if any differs
int features_differ(const W (&col)[C], const int (&h)[C], int R) {
  int bad = 0;
  int f[6], g[6];
  tet::board_features<W, C, 0, 12>(col, h, R, kLut12.bytes, f[0], f[1], f[2], f[3], f[4], f[5]);
  tet::board_features_parent<W, C, 0, 12>(col, h, R, kLut12.bytes, g[0], g[1], g[2], g[3], g[4], g[5]);
  bad |= memcmp(f, g, sizeof(f)) != 0;
  if (R <= 20) {  // the 10-row-chunk tables of the stepping kernels
    tet::board_features<W, C, 2, 10>(col, h, R, kLut10.bytes, f[0], f[1], f[2], f[3], f[4], f[5]);
    tet::board_features_parent<W, C, 2, 10>(col, h, R, kLut10.bytes, g[0], g[1], g[2], g[3], g[4], g[5]);
    bad |= memcmp(f, g, sizeof(f)) != 0;
  }
  return bad;
}

}  // namespace

extern "C" {

// Set (i): rows R-4 .. R-1 of a 6-column window run through patterns (every `every`-th of the 2^24, offset by a
// hash so that no bit is fixed), the window at every position 0 .. C-6; the other columns' top rows and every
// row below R-4 are random (fixed seed); no cell at or above R.  Every piece of the set, full 48-bit mask.
// The present top-rows mask against the parent's top-rows AND general forms; board_features in both table variants
// against the parent's.  Returns the number of mask mismatches; rescued[i] += rescued placements seen for piece i;
// *checked += masks compared; *feat_bad += boards whose features differ.
int64_t lane_vm_window(int R, int n_pieces, const int32_t* piece_ids, uint64_t seed, int every, int64_t* rescued,
                       int64_t* checked, int64_t* feat_bad) {
  Tables t;
  make_tables(n_pieces, piece_ids, &t);
  int64_t bad = 0, n_chk = 0, bad_f = 0;
  int64_t resc[16] = {0};
  const int64_t n_pat = ((int64_t)1 << 24) / every;
#pragma omp parallel for schedule(static) reduction(+ : bad, n_chk, bad_f) reduction(+ : resc[:16])
  for (int64_t q = 0; q < n_pat; ++q) {
    const uint32_t pat = (uint32_t)(q * every + (int64_t)(mix64(seed ^ (uint64_t)q) % (uint64_t)every));
    for (int pos = 0; pos + 6 <= C; ++pos) {
      const uint64_t r0 = mix64(seed * 31 + (uint64_t)pat * 8 + (uint64_t)pos);
      W col[C];
      int h[C];
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
      tet::heights_of<W, C>(col, h);
      for (int i = 0; i < n_pieces; ++i) {
        const uint64_t a = tet::valid_mask<W, C, true>(col, h, t.now.orient[i], t.now.fullmask[i], R);
        const uint64_t b = tet::valid_mask_parent<W, C, true>(col, h, t.now.orient[i], t.now.fullmask[i], R);
        bad += (a != b);
        bad += (a != tet::valid_mask_parent<W, C, false>(col, h, t.now.orient[i], t.now.fullmask[i], R));
        ++n_chk;
        resc[i] += count_rescued(b, tet::kCatalogue[piece_ids[i]], h, R);
      }
      bad_f += features_differ(col, h, R);
    }
  }
  for (int i = 0; i < n_pieces; ++i) rescued[i] += resc[i];
  *checked += n_chk;
  *feat_bad += bad_f;
  return bad;
}

// Sets (ii), (iii): given boards (ten column words each).  valid_mask for every piece of the set in both of the
// present forms (TOP as env_step calls it, and the general one refresh_kernel keeps) against the parent's, and
// board_features in the table variants the kernels instantiate for R.  out[0] += mask mismatches, out[1] +=
// feature mismatches, out[2] += boards with a cell at or above R (the caller asserts 0), out[3] += masks compared,
// out[4] += wavefronts (64 consecutive boards) whose rescue evaluation runs, out[5] += wavefronts, out[6] +=
// wavefronts in which the sharper (unbuilt) rescue test would still run.
void lane_boards(int R, int n_pieces, const int32_t* piece_ids, const uint32_t* cols, int64_t n, int64_t* out) {
  Tables t;
  make_tables(n_pieces, piece_ids, &t);
  int64_t bad_m = 0, bad_f = 0, dirty = 0, n_chk = 0, wav_run = 0, wav = 0, wav_sharp = 0;
#pragma omp parallel for schedule(static) reduction(+ : bad_m, bad_f, dirty, n_chk, wav_run, wav, wav_sharp)
  for (int64_t w0 = 0; w0 < n; w0 += 64) {
    bool any = false, any_sharp = false;
    for (int64_t b = w0; b < w0 + 64 && b < n; ++b) {
      W col[C];
      int h[C];
      for (int c = 0; c < C; ++c) col[c] = cols[b * C + c];
      tet::heights_of<W, C>(col, h);
      bool over = false;
      int n3 = 0;
      for (int c = 0; c < C; ++c) {
        over |= (col[c] >> R) != 0;
        n3 += h[c] >= R - 2;
      }
      if (over) {
        ++dirty;
        continue;
      }
      any |= n3 >= C - 4;
      // the sharper rescue test the issue proposes (NOT built): a row among R-3 .. R-1 can be completed by a
      // piece only if its missing cells span at most four adjacent columns
      for (int t = 0; t < 3; ++t) {
        uint32_t m = 0;
        for (int c = 0; c < C; ++c) m |= (uint32_t)(((col[c] >> (R - 3 + t)) & 1u) ^ 1u) << c;
        if (m != 0 && (31 - __builtin_clz(m)) - __builtin_ctz(m) <= 3) any_sharp = true;
      }
      for (int i = 0; i < n_pieces; ++i) {
        const uint64_t r = tet::valid_mask_parent<W, C, true>(col, h, t.now.orient[i], t.now.fullmask[i], R);
        bad_m += tet::valid_mask<W, C, true>(col, h, t.now.orient[i], t.now.fullmask[i], R) != r;
        bad_m += tet::valid_mask<W, C, false>(col, h, t.now.orient[i], t.now.fullmask[i], R) != r;
        bad_m += tet::valid_mask_parent<W, C, false>(col, h, t.now.orient[i], t.now.fullmask[i], R) != r;
        ++n_chk;
      }
      bad_f += features_differ(col, h, R);
    }
    ++wav;
    wav_run += any;
    wav_sharp += any_sharp;
  }
  out[0] += bad_m;
  out[1] += bad_f;
  out[2] += dirty;
  out[3] += n_chk;
  out[4] += wav_run;
  out[5] += wav;
  out[6] += wav_sharp;
}

}  // extern "C"
