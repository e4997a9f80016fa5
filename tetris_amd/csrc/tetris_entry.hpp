// tetris_entry.hpp -- what a kernel of tetris_kernels.hip and the CPU entry of the same name in
// tests/harness/core_host.cpp share beyond the lane logic of tetris_core.hpp: which template
// instantiation runs for a geometry, the table blobs, the per-env bodies that are not a step, and the
// parameter blocks the C-ABI (tetris_abi.inc) fills for both.
// The kernels add what only a GPU needs (LDS staging, ballots, paired stores, launch bounds).
#pragma once
#include "tetris_core.hpp"
#include "tetris_table.hpp"
#if !defined(__HIPCC__)
#include <math.h>  // expf / logf of the softmax policy's CPU twin (the device has its own)
#endif

#ifndef TET_LUT10
#define TET_LUT10 1   // 0: always the 12-row-chunk tables (A/B timing)
#endif
#if defined(__HIPCC__)
#define TET_TABLE __device__ const
#else
#define TET_TABLE const
#endif

namespace {  // (one copy per translation unit, under the names the kernels' code objects have always carried)

// feature tables (tools/gen_feature_lut.py): byte tables for hole depth and wells (28 KiB), copied
// to LDS as one block by the kernels that compute features
struct alignas(16) FeatureLut {
  uint8_t bytes[tet::kFeatureLutBytes];
};
TET_TABLE FeatureLut kFeatureLut = {{
#include "tetris_feature_lut.inc"
}};
static_assert(sizeof(FeatureLut) == tet::kFeatureLutBytes, "layout assumed by col_wells");
// the same tables for 10-row chunks (7 KiB): stepping kernels on boards of up to 20 rows
struct alignas(16) FeatureLut10 {
  uint8_t bytes[tet::kFeatureLut10Bytes];
};
TET_TABLE FeatureLut10 kFeatureLut10 = {{
#include "tetris_feature_lut10.inc"
}};
// tables of the kernels that walk the afterstates (tet::AfterLut: hole tables, packed wells entries, select tables)
struct alignas(16) AfterLutData {
  uint8_t bytes[tet::kAfterLutBytes];
};
TET_TABLE AfterLutData kAfterLut = {{
#include "tetris_after_lut.inc"
}};

}  // namespace

namespace tet {

template <bool V> struct BoolConst { static constexpr bool value = V; };

// Where a hot kernel (step, step_many, rollouts) still writes one of the small bodies below out itself,
// sharing it moved the kernel's device code (operand order, register allocation), and that code is held
// fixed; the text there is the same rule and the CPU entry calls the function here.

// ---- kernel variant of a geometry ---------------------------------------------------------------
// Packed boards (tet::board_packed: stored rows within three quarters of the word) always run the
// variants with a compile-time chunk count -- NCH = 2 on u32, 4 on u64 -- and those variants read /
// write the packed planes; everything else is NCH = 0 on one plane per column.
template <typename W>
inline bool packed_geometry(int R) { return R + 4 <= 6 * (int)sizeof(W); }  // == tet::board_packed (TET_NO_PACK builds keep the variant choice)
template <typename W>
constexpr int packed_chunks() { return sizeof(W) == 4 ? 2 : 4; }

// The ONE place that turns (W, R) into template arguments: f(IntConst<NCH>, IntConst<CR>, BoolConst<PACK>).
// The stepping kernels take (NCH, CR), the afterstate family NCH (its tables are the 12-row AfterLut), reset
// and refresh PACK.  CR: a step only evaluates the features of a NON-terminal board (cells below row R): up to
// R = 20 (u32) two 10-row chunks cover it, up to R = 40 (u64) four, and the tables are the 7 KiB set;
// otherwise 12-row chunks.
template <typename W, typename F>
inline void kernel_variant(int R, F&& f) {
  constexpr int N = packed_chunks<W>();
  if (!packed_geometry<W>(R)) f(IntConst<0>{}, IntConst<12>{}, BoolConst<false>{});
  else if (R <= 10 * N && TET_LUT10) f(IntConst<N>{}, IntConst<10>{}, BoolConst<!TET_NO_PACK>{});
  else f(IntConst<N>{}, IntConst<12>{}, BoolConst<!TET_NO_PACK>{});
}

// ---- a step's configuration -----------------------------------------------------------------------
inline void fill_step_cfg(StepCfg& cfg, const TetrisDesc* desc, int auto_reset, bool compute_obs) {
  cfg.R = desc->num_rows;
  cfg.n_pieces = desc->n_pieces;
  cfg.auto_reset = auto_reset;
  cfg.compute_obs = compute_obs;
  cfg.has_direct_by = desc->has_direct_by;
  for (int i = 0; i < 8; ++i) cfg.direct_by[i] = desc->direct_by[i];
}
// the two keys of step `step_idx` (four counters per step: + 2 is the reset's, + 1 is free)
TET_HD void step_keys(uint64_t seed, uint64_t step_idx, StepCfg& cfg) {
  cfg.key_step = hash_key(seed, step_idx * 4u + 0u);
  cfg.key_policy = hash_key(seed, step_idx * 4u + 3u);
}

// ---- replay stream ------------------------------------------------------------------------------
// What env i of B reads for one step from `stream` ([stream_len][B] piece indices, NULL: none) at its
// cursor: the piece of the step draw and of the reset draw.  A step consumes one row, two when it
// ends the episode under auto-reset: an env whose stream cannot cover that is `exhausted` -- counted
// as invalid and left untouched (never a silent replay of the last row).
TET_HD void stream_read(const uint8_t* stream, const int32_t* cursors, int64_t stream_len, int64_t B, int64_t i,
                        const StepCfg& cfg, int& draw, int& draw_reset, int& cursor, bool& exhausted) {
  draw = -1;
  draw_reset = -1;
  cursor = 0;
  exhausted = false;
  if (stream) {
    cursor = cursors[i];
    exhausted = (int64_t)cursor + (cfg.auto_reset ? 2 : 1) > stream_len || cursor < 0;
    int64_t r0 = cursor < stream_len ? cursor : stream_len - 1;
    int64_t r1 = cursor + 1 < stream_len ? cursor + 1 : stream_len - 1;
    draw = stream[r0 * B + i];
    draw_reset = stream[r1 * B + i];
  }
}
// the cursor after a step that was not invalid
TET_HD int stream_advance(int cursor, const StepOut& out, const StepCfg& cfg) {
  return cursor + 1 + ((out.done && cfg.auto_reset) ? 1 : 0);
}
// a reset consumes one row: an env whose cursor is at or past the end is left untouched and counted
// as invalid (as the step does), never continued on the last row
TET_HD bool stream_reset_exhausted(int cursor, int64_t stream_len) { return cursor < 0 || cursor >= stream_len; }

// ---- reset / refresh of one env -------------------------------------------------------------------
// game.py:53-63: empty board, a piece from the stream row at `cursor` or from the (fresh or kept) bag
template <typename W, int C, bool PACK>
TET_HD void reset_env(W* cols, uint64_t* meta, int64_t B, int64_t i, const SetTable& tab, int init_bag, int n_pieces,
                      uint32_t key, int64_t env_offset, const uint8_t* stream, int32_t* cursors, int cursor,
                      uint8_t* piece_out, uint8_t* n_valid_out) {
#pragma unroll
  for (int q = 0; q < n_planes(C, PACK); ++q) cols[plane_index(i, q, n_planes(C, PACK))] = 0;  // game.py:55-58
  uint32_t bag = init_bag ? 0u : meta_bag(meta[i]);
  int piece;
  if (stream) {
    piece = stream[(int64_t)cursor * B + i];
    cursors[i] = cursor + 1;
  } else {
    piece = bag_draw(bag, n_pieces, hash_env(key, (uint32_t)(env_offset + i)) >> 16);  // game.py:60
  }
  const uint64_t mask = tab.fullmask[piece];
  meta[i] = meta_pack(mask, piece, bag);
  if (piece_out) piece_out[i] = (uint8_t)piece;
  if (n_valid_out) n_valid_out[i] = (uint8_t)popc(mask);
}

// the valid mask of env i's board for the piece its control word names, recomputed
template <typename W, int C, bool PACK>
TET_HD void refresh_env(const W* cols, uint64_t* meta, uint8_t* n_valid_out, int64_t B, int64_t i, const SetTable& tab,
                        int R) {
  W col[C];
  int h[C];
  load_board<W, C, PACK>(cols, B, i, col);
  heights_of<W, C>(col, h);
  const uint64_t m = meta[i];
  const int piece = meta_piece(m);
  const uint64_t mask = valid_mask<W, C>(col, h, piece_entries(tab, piece), tab.fullmask[piece], R);
  meta[i] = meta_pack(mask, piece, meta_bag(m));
  if (n_valid_out) n_valid_out[i] = (uint8_t)popc(mask);
}

// ---- copy of one env between batches ----------------------------------------------------------------
// dst env j := src env idx (tetris_hip_gather_envs) on the stored representation: the n_planes words of the
// board, whatever they pack, and all 64 bits of meta -- mask, piece and bag.  idx == -1 keeps env j; any other
// idx outside [0, B_src) keeps it too and is reported (returns true).  NP, the plane count, is a template
// argument so that the loads are one straight run issued before the first store (with NP a launch argument and a
// guard per plane of an unrolled loop the compiler put a wait on the previous store in front of every store).
constexpr int kMetaPieces = 16;  // a fullmask entry for every value of meta's 4-bit piece field
template <typename W, int NP>
TET_HD bool gather_env(const W* src_cols, const uint64_t* src_meta, int64_t B_src, W* dst_cols, uint64_t* dst_meta,
                       uint8_t* dst_n_valid, uint8_t* dst_piece, int32_t idx, int64_t j, const uint64_t* fullmask) {
  if (idx == -1) return false;
  if (idx < 0 || idx >= B_src) return true;
  const W* s = src_cols + plane_index(idx, 0, NP);
  W w[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) w[q] = s[q * kTileEnvs];
  const uint64_t m = src_meta[idx];
  W* d = dst_cols + plane_index(j, 0, NP);
#pragma unroll
  for (int q = 0; q < NP; ++q) d[q * kTileEnvs] = w[q];
  dst_meta[j] = m;
  const int piece = meta_piece(m);
  if (dst_n_valid) dst_n_valid[j] = (uint8_t)popc(meta_mask(m) & fullmask[piece]);
  if (dst_piece) dst_piece[j] = (uint8_t)piece;
  return false;
}
// f(IntConst<NP>) for the plane count of a geometry: 4 (five packed columns) to 12 (twelve unpacked)
template <typename F>
inline bool gather_variant(int np, F&& f) {
  switch (np) {
#define TET_X(N) case N: f(IntConst<N>{}); return true;
    TET_X(4) TET_X(5) TET_X(6) TET_X(7) TET_X(8) TET_X(9) TET_X(10) TET_X(11) TET_X(12)
#undef TET_X
    default: return false;
  }
}

// ---- expansion of envs into their afterstates --------------------------------------------------------
// dst env j := src env parent[j] after placement action[j] (tetris_hip_expand_envs): what a step without auto-reset
// makes of the parent, written to ANOTHER batch, with the next piece either dictated (next_piece, env_step's replay
// `draw`: the bag is kept) or drawn from the parent's bag under the parent's env id.  An entry is kept (parent == -1:
// nothing written, nothing counted), run, or bad (any other parent outside [0, B_src), a piece outside the set: nothing
// written, counted); a run entry whose action is no placement of the parent -- every action of a parent that is over --
// comes back from the body with out.invalid set and is bad too.
enum { kExpandKeep = 0, kExpandRun = 1, kExpandBad = 2 };
TET_HD int expand_entry(int32_t parent, uint32_t B_src, int next_piece, int n_pieces) {
  if (parent == -1) return kExpandKeep;
  return (parent < 0 || (uint32_t)parent >= B_src || next_piece >= n_pieces) ? kExpandBad : kExpandRun;
}
// the per-env body on the parent's unpacked board and meta: col / meta become the child's unless out.invalid.
// next_piece < 0: drawn.  `env` is the PARENT's global id, so every child of one parent draws the same piece.
template <typename W, int C, int NCH, int CR, bool SPAD>
TET_HD void expand_env(W (&col)[C], uint64_t& meta, int action, int next_piece, const SetTable& tab, const uint8_t* lut,
                       W* scratch, int sstride, const StepCfg& cfg, uint32_t env, StepOut& out) {
  env_step<W, C, NCH, CR, false, SPAD>(col, meta, action, false, tab, lut, scratch, sstride, cfg, env, next_piece, -1, out);
}

// ---- rollout fan-out ------------------------------------------------------------------------------
// Mean return of the n rollouts of (env i, first action a0); NaN where a0 is not an action of the env.
// Rollout r has the global id uid (its low word keys the hashes, its high word the key) and reads its
// fed pieces, if any, from pieces[i][a0][r][0 .. length).
template <typename W, int C, int NCH>
TET_HD double rollout_mean(const W (&col)[C], uint64_t meta, int64_t i, int a0, int64_t env_offset, int a_max, int n,
                           int length, int policy, const float (&w)[8], const SetTable& tab, const uint8_t* lut,
                           W* scratch, int sstride, int R, int n_pieces, uint32_t key, const uint8_t* pieces) {
  const int nv = popc(meta_mask(meta));
  double mean = __builtin_nan("");
  if (a0 < nv) {
    int sum = 0;
    for (int r = 0; r < n; ++r) {
      const uint64_t uid = ((uint64_t)(env_offset + i) * (uint64_t)a_max + (uint64_t)a0) * (uint64_t)n + r;
      const uint32_t key0 = mix32(key ^ ((uint32_t)(uid >> 32) * 0x9E3779B1u));
      const uint64_t fed = ((uint64_t)(i * a_max + a0) * (uint64_t)n + (uint64_t)r) * (uint64_t)length;
      sum += rollout_env<W, C, NCH>(col, meta, a0, length, policy, w, tab, lut, scratch, sstride, R, n_pieces, key0,
                                    (uint32_t)uid, pieces ? pieces + fed : nullptr);
    }
    mean = (double)sum / (double)n;
  }
  return mean;
}

// ---- greedy play of a population of linear policies ---------------------------------------------------
// (tetris_hip_policy_greedy_rows / tetris_hip_play_linear): env i evaluates with row rows[i] of a DEVICE matrix
// weights[P][8] (without a row list: row i).  A row outside [0, P) leaves the env alone and is reported.
TET_HD bool weight_row_ok(int32_t row, int32_t P) { return row >= 0 && row < P; }
// the eight weights of one row: two 16-byte loads (rows are 32 bytes, the matrix 16-byte aligned); lanes that
// share a row read the same 32 bytes
TET_HD void load_weight_row(const float* weights, int32_t row, float (&w)[8]) {
#if defined(__HIPCC__)
  const float4* src = reinterpret_cast<const float4*>(weights) + 2 * (int64_t)row;
  const float4 lo = src[0], hi = src[1];
  w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w;
  w[4] = hi.x, w[5] = hi.y, w[6] = hi.z, w[7] = hi.w;
#else
  for (int q = 0; q < 8; ++q) w[q] = weights[(int64_t)row * 8 + q];
#endif
}
// the greedy policy's choice for one env (game.py:102-120 on the non-terminal placements): fitness_of on the
// features of the afterstate walk, GreedyPick's first maximum.  `lut` is an AfterLut.
template <typename W, int C, int NCH>
TET_HD GreedyPick greedy_pick_env(const W (&col)[C], uint64_t meta, const SetTable& tab, const uint8_t* lut, int R,
                                  const float (&w)[8]) {
  GreedyPick pick;
  afterstates_env<W, C, NCH>(col, meta, tab, lut, R, [&](bool has, int, int, float (&f)[8], int, int row, bool is_valid) {
    if (has && is_valid) pick.offer(fitness_of(f, w), row);
  });
  return pick;
}
// an env is over when its current piece has no non-terminal placement (env_step's n_valid == 0): play freezes it
TET_HD bool env_over(uint64_t meta) { return popc(meta_mask(meta)) == 0; }
// one greedy step of an env that is not over: the pick, then the step on the afterstate family's tables
// (12-row chunks), exactly what step_many's greedy variant runs per step.  SPAD as env_step's.
template <typename W, int C, int NCH, bool SPAD>
TET_HD void play_step_env(W (&col)[C], uint64_t& meta, const float (&w)[8], const SetTable& tab, const uint8_t* lut,
                          W* scratch, int sstride, const StepCfg& cfg, uint32_t env, StepOut& out) {
  const GreedyPick pick = greedy_pick_env<W, C, NCH>(col, meta, tab, lut, cfg.R, w);
  env_step<W, C, NCH, 12, true, SPAD>(col, meta, pick.best_row, false, tab, lut, scratch, sstride, cfg, env, -1, -1, out);
}

// ---- two-piece lookahead ---------------------------------------------------------------------------------
// (tetris_hip_policy_two_ply)  The pieces the sum of an env runs over: its bag (meta bits 52-63) within the set; an
// empty bag is the whole set, as bag_draw refills it.
TET_HD uint32_t two_ply_bag(uint64_t meta, int n_pieces) {
  const uint32_t all = (1u << n_pieces) - 1u;
  const uint32_t bag = meta_bag(meta) & all;
  return bag ? bag : all;
}
// the first actions of an env: the placements its mask holds (env_step's count), never more than a row of q has
TET_HD int two_ply_n_valid(uint64_t meta, int a_max) {
  const int nv = popc(meta_mask(meta));
  return nv < a_max ? nv : a_max;
}
// One (env, first action k): placement k of the current piece is stamped once -- land, lock, clear: env_step, as
// tetris_hip_step and expand_env run it, with the next piece dictated so that nothing is drawn -- and every piece p of
// the set is then evaluated on that board: its valid mask as env_step computes the drawn piece's, greedy_pick_env on
// it.  value[p] = the pick's best, -inf where piece p has no non-terminal placement; written to values_row[p] when
// given.  Returns q: the float32 sum, in ascending p from the first term, of value[p] over the pieces of `bag` with
// -inf replaced by death_value.  k is no placement of the env: NaN, in the row too.  col is consumed (it becomes the
// child's board).  `lut` is an AfterLut; SPAD as env_step's.
template <typename W, int C, int NCH, bool SPAD>
TET_HD float two_ply_lane(W (&col)[C], uint64_t meta, int k, uint32_t bag, const float (&w)[8], float death_value,
                          int n_pieces, const SetTable& tab, const uint8_t* lut, W* scratch, int sstride, int R,
                          float* values_row) {
  const float nan = __builtin_nanf(""), ninf = -__builtin_inff();
  if (k >= popc(meta_mask(meta))) {
    if (values_row)
      for (int p = 0; p < n_pieces; ++p) values_row[p] = nan;
    return nan;
  }
  StepCfg cfg;
  cfg.R = R;
  cfg.n_pieces = n_pieces;
  cfg.auto_reset = 0;
  cfg.key_step = cfg.key_policy = 0u;
  cfg.compute_obs = 0;
  cfg.has_direct_by = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) cfg.direct_by[j] = 1.0f;
  StepOut out;
  env_step<W, C, NCH, 12, true, SPAD>(col, meta, k, false, tab, lut, scratch, sstride, cfg, 0u, 0, -1, out);
  int h[C];
  heights_of<W, C>(col, h);
  float q = 0.f;
  bool first = true;
#pragma unroll 1
  for (int p = 0; p < n_pieces; ++p) {
    const uint64_t mask = valid_mask<W, C, (sizeof(W) == 4 && C <= 10)>(col, h, piece_entries(tab, p), tab.fullmask[p], R);
    const GreedyPick pick = greedy_pick_env<W, C, NCH>(col, meta_pack(mask, p, 0u), tab, lut, R, w);
    const float v = pick.best_row < 0 ? ninf : pick.best;
    if (values_row) values_row[p] = v;
    if ((bag >> p) & 1u) {
      const float t = v == ninf ? death_value : v;
      q = first ? t : TET_FADD(q, t);
      first = false;
    }
  }
  return q;
}
// the pick of one env over its row of sums: GreedyPick's first maximum over the n_valid entries in ascending k (all
// -inf: action 0; no entry: action -1, value 0)
TET_HD GreedyPick two_ply_pick(const float* q_row, int n_valid) {
  GreedyPick pick;
  for (int k = 0; k < n_valid; ++k) pick.offer(q_row[k], k);
  return pick;
}

// ---- softmax linear policy: sample, log-probability and score -----------------------------------------
// (tetris_hip_policy_softmax_rows / tetris_hip_play_softmax; utils.py:26-38 of the reference:
// compute_action_probabilities and grad_of_log_action_probabilities.)  One pass over afterstates_env, as
// greedy_pick_env; no row of logits is stored and there is no second pass.  For the non-terminal placement with
// row index k (the action it is), features f -- multiplied by direct_by when the descriptor has it, i.e. the row
// tetris_hip_afterstates writes; the greedy calls evaluate undirected features -- and weights w:
//   logit       u_k = fitness_of(f, w) * inv_t           float32, left to right, inv_t = 1.0f / temperature
//   online log-sum-exp and expectation over the placements IN THE ORDER THE WALK EMITS THEM:
//               d = u_k - m;  e = expf(-|d|);  (r, a) = d > 0 ? (e, 1) : (1, e)
//               s = s * r + a;   g[q] = g[q] * r + a * f[q];   m = max(m, u_k)       (m = -inf, s = 0, g = 0 first)
//     every product and sum rounded to float32 on its own.  The walk emits the placements that complete a row
//     AFTER all the others, not in row order, so s and g are float32 sums in that order: the results are
//     reproducible for a given board, but NOT independent of the order (two boards with the same logits in
//     another emission order may differ in the last bits).
//   Gumbel-max draw:   h_k = hash_env(mix32(key ^ ((uint32_t)(k + 1) * 0x9E3779B1u)), env)
//               U_k = ((h_k >> 8) + 1) * 2^-24   in (0, 1], exact in float32
//               z_k = u_k - logf(-logf(U_k))               (U_k = 1: z_k = +inf)
//     with key = hash_key(seed, 4 * step_idx + 1) -- the counter of a step that step_keys leaves free -- and
//     env the global env index mod 2^32.  The action is the row of maximal z; of exactly equal z the lower row
//     (GreedyPick's rule).  The picked row's u and f are kept.
//   results     logz = m + logf(s);  logp = (u_a - m) - logf(s);  score[q] = f_a[q] - g[q] / s
//     (logp is u_a - logz evaluated in the order that does not cancel: with logits in the thousands u_a - logz in
//     float32 is good to 1e-3 absolute, (u_a - m) - logf(s) to an ulp of logp)
//     score is grad_of_log_action_probabilities (utils.py:34-38): the gradient of log p(a) with respect to the
//     weights WITHOUT the factor 1 / temperature, as upstream.
// An env without a non-terminal placement: action -1, logp = logz = 0, score = 0.  With one placement s = 1 and
// g = f exactly, so logp = 0 and score = 0 exactly.  The logits must be finite.
struct SoftmaxPick {
  int action;
  float logp, logz;
  float score[8];
};
TET_HD uint32_t softmax_key(uint64_t seed, uint64_t step_idx) { return hash_key(seed, step_idx * 4u + 1u); }
// logits_row: NULL or the env's row of a_max floats: entry k = u_k is written for k < n_valid (the caller pads)
template <typename W, int C, int NCH>
TET_HD void softmax_pick_env(const W (&col)[C], uint64_t meta, const SetTable& tab, const uint8_t* lut, int R,
                             const float (&w)[8], float inv_t, bool directed, const float (&direct_by)[8], uint32_t key,
                             uint32_t env, float* logits_row, SoftmaxPick& out) {
  float m = -__builtin_inff(), s = 0.f, g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float z_best = 0.f, u_a = 0.f, f_a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int best_row = -1;
  afterstates_env<W, C, NCH>(col, meta, tab, lut, R, [&](bool has, int, int, float (&f)[8], int, int row, bool is_valid) {
    if (!(has && is_valid)) return;
    if (directed) {
#pragma unroll
      for (int q = 0; q < 8; ++q) f[q] = TET_FMUL(f[q], direct_by[q]);
    }
    const float u = TET_FMUL(fitness_of(f, w), inv_t);
    if (logits_row) logits_row[row] = u;
    const float d = u - m;
    const float e = expf(-fabsf(d));
    const bool up = d > 0.f;
    const float r = up ? e : 1.f, a = up ? 1.f : e;
    s = TET_FADD(TET_FMUL(s, r), a);
#pragma unroll
    for (int q = 0; q < 8; ++q) g[q] = TET_FADD(TET_FMUL(g[q], r), TET_FMUL(a, f[q]));
    m = up ? u : m;
    const uint32_t h = hash_env(mix32(key ^ ((uint32_t)(row + 1) * 0x9E3779B1u)), env);
    const float U = TET_FMUL((float)((h >> 8) + 1u), 5.9604644775390625e-08f);  // 2^-24
    const float z = u - logf(-logf(U));
    if (best_row < 0 || z > z_best || (z == z_best && row < best_row)) {
      z_best = z;
      best_row = row;
      u_a = u;
#pragma unroll
      for (int q = 0; q < 8; ++q) f_a[q] = f[q];
    }
  });
  out.action = best_row;
  if (best_row < 0) {
    out.logp = out.logz = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) out.score[q] = 0.f;
  } else {
    const float log_s = logf(s);
    out.logz = TET_FADD(m, log_s);
    out.logp = (u_a - m) - log_s;  // not u_a - logz: that subtraction cancels at the size of the logits
#pragma unroll
    for (int q = 0; q < 8; ++q) out.score[q] = f_a[q] - g[q] / s;
  }
}
// one sampled step of an env that is not over: the draw, then the step (as play_step_env)
template <typename W, int C, int NCH, bool SPAD>
TET_HD void play_softmax_step_env(W (&col)[C], uint64_t& meta, const float (&w)[8], float inv_t, uint32_t key_sample,
                                  const SetTable& tab, const uint8_t* lut, W* scratch, int sstride, const StepCfg& cfg,
                                  uint32_t env, SoftmaxPick& pick, StepOut& out) {
  softmax_pick_env<W, C, NCH>(col, meta, tab, lut, cfg.R, w, inv_t, cfg.has_direct_by != 0, cfg.direct_by, key_sample, env,
                              nullptr, pick);
  env_step<W, C, NCH, 12, true, SPAD>(col, meta, pick.action, false, tab, lut, scratch, sstride, cfg, env, -1, -1, out);
}

// ---- the reference's piece sampler on NumPy's legacy global stream ----------------------------------
// (tetromino.py:12-22 on top of np.random.seed / np.random.permutation): env i is
// seeded like `np.random.seed(seeds[i])` right before `game.Tetris(...)` is constructed, and row t of
// the stream is the list index its sampler hands out at its t-th call.  MT19937 (Matsumoto &
// Nishimura) with NumPy's init_genrand seeding; permutation(n) = Fisher-Yates from the top with
// masked rejection sampling on raw 32-bit outputs.  The 2.5 KB generator state is private to the env.
TET_HD void numpy_bag_stream_env(const uint32_t* seeds, int n_pieces, int64_t L, uint8_t* stream, int64_t B, int64_t i) {
  uint32_t mt[624];
  mt[0] = seeds[i];
  for (int k = 1; k < 624; ++k) mt[k] = 1812433253U * (mt[k - 1] ^ (mt[k - 1] >> 30)) + (uint32_t)k;
  int pos = 624;
  auto next_u32 = [&]() -> uint32_t {
    if (pos >= 624) {
      for (int k = 0; k < 624; ++k) {
        const uint32_t y = (mt[k] & 0x80000000U) | (mt[k + 1 < 624 ? k + 1 : 0] & 0x7fffffffU);
        mt[k] = mt[k + 397 < 624 ? k + 397 : k + 397 - 624] ^ (y >> 1) ^ ((y & 1U) ? 0x9908b0dfU : 0U);
      }
      pos = 0;
    }
    uint32_t y = mt[pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680U;
    y ^= (y << 15) & 0xefc60000U;
    y ^= y >> 18;
    return y;
  };
  uint8_t bag[TETRIS_MAX_PIECES];
  int left = 0;
  for (int64_t t = 0; t < L; ++t) {
    if (left == 0) {  // tetromino.py:15,18-19: a fresh np.random.permutation(n)
      for (int k = 0; k < n_pieces; ++k) bag[k] = (uint8_t)k;
      for (int k = n_pieces - 1; k >= 1; --k) {
        uint32_t mask = (uint32_t)k;
        mask |= mask >> 1;
        mask |= mask >> 2;
        mask |= mask >> 4;
        uint32_t v;
        do {
          v = next_u32() & mask;
        } while (v > (uint32_t)k);
        const uint8_t tmp = bag[k];
        bag[k] = bag[v];
        bag[v] = tmp;
      }
      left = n_pieces;
    }
    stream[t * B + i] = bag[n_pieces - left];  // tetromino.py:20-21: element 0, then delete it
    --left;
  }
}

}  // namespace tet

// ---- parameter blocks -------------------------------------------------------------------------------
// What the C-ABI (tetris_abi.inc) fills and a launch takes: the kernels by value, the CPU entries by reference.
namespace {  // (as the table blobs above: the kernels' mangled names carry these types)

struct StepParams {
  void* cols;              // tile-major board words (tet::plane_index)
  uint64_t* meta;
  const int32_t* action;   // NULL: built-in uniform random policy
  int32_t* action_out;     // optional: the action each env played
  const uint8_t* stream;
  int32_t* cursor;
  int64_t stream_len;
  float* obs;
  int32_t* reward;
  uint8_t* done;
  uint8_t* lines;
  uint8_t* n_valid;
  uint8_t* piece_next;
  uint32_t* status;
  // payload of the done/reset gather, written by the step itself when given: one 64-bit done
  // mask per wavefront (bit = lane) and a copy of the wavefront's counter slot as of THIS step -- a
  // consistent snapshot in memory no later step touches, so the exchange can run beside the next steps
  unsigned long long* done_bits;
  uint32_t* status_snapshot;
  uint32_t B;
  uint32_t env_offset;     // global env index of env 0 (mod 2^32)
  // step index from device memory (HIP-graph replays: the kernel arguments of a captured launch are
  // frozen, the step's hash keys must not be): when set, the keys are derived in the kernel from
  // *step_counter + step_rel instead of taken from cfg
  const uint64_t* step_counter;
  uint64_t seed;
  uint32_t step_rel;
  tet::StepCfg cfg;
  tet::SetTable tab;
};

struct StepManyParams {
  StepParams one;        // pointers of step 0; per-step outputs advance by B elements per step
  int32_t n_steps;
  int32_t policy;        // 0 uniform random, 1 greedy on w
  uint64_t seed;
  uint64_t step_idx0;
  float w[8];
};

struct ResetParams {
  void* cols;
  uint64_t* meta;
  uint32_t* status;        // per-wave counters or NULL: an env whose replay stream is exhausted is counted as invalid
  const uint8_t* reset_mask;
  uint8_t* piece_out;
  uint8_t* n_valid_out;
  const uint8_t* stream;
  int32_t* cursor;
  int64_t stream_len;
  int64_t B;
  int64_t env_offset;
  int32_t init_bag;
  int32_t n_pieces;
  int32_t R;
  uint32_t key;
  tet::SetTable tab;
};

struct RefreshParams {
  const void* cols;
  uint64_t* meta;
  uint8_t* n_valid_out;
  int64_t B;
  int32_t R;
  tet::SetTable tab;
};

struct AfterParams {
  const void* cols;
  const uint64_t* meta;
  float* feats;
  uint8_t* n_valid;
  float* feats_all;
  uint8_t* n_all;
  int64_t B;
  int64_t env_stride;  // in floats: distance between the matrices of consecutive envs
  int64_t row_stride;  // in floats: distance between consecutive feature rows of one env
  int32_t R;
  int32_t a_max;
  int32_t has_direct_by;
  float direct_by[8];
  tet::SetTable tab;
};

struct GreedyParams {
  const void* cols;
  const uint64_t* meta;
  int32_t* best_action;
  float* best_value;
  float* fitness_all;
  int64_t B;
  int32_t R;
  int32_t a_max;
  float w[8];
  tet::SetTable tab;
};

struct RolloutParams {
  const void* cols;
  const uint64_t* meta;
  double* returns;  // [B][a_max]
  int64_t B;
  int64_t env_offset;
  int32_t R;
  int32_t a_max;
  int32_t n_pieces;
  int32_t length;
  int32_t n;
  int32_t policy;
  uint32_t key;
  const uint8_t* pieces;  // NULL, or uint8 [B][a_max][n][length]: the piece every step of every rollout draws
  float w[8];
  tet::SetTable tab;
};

struct GreedyRowsParams {
  const void* cols;
  const uint64_t* meta;
  const float* weights;    // DEVICE [P][8], 16-byte aligned
  const int32_t* rows;     // [B]: the weight row of each env, or NULL: env i uses row i
  int32_t* best_action;
  float* best_value;       // optional
  uint32_t* status;        // per-wave counters or NULL: an env whose row is outside [0, P) is counted as invalid
  int64_t B;
  int32_t P;
  int32_t R;
  tet::SetTable tab;
};

struct PlayParams {
  void* cols;
  uint64_t* meta;
  const float* weights;    // as GreedyRowsParams
  const int32_t* rows;
  uint32_t* lines_total;   // [B], added to
  uint32_t* pieces_total;  // [B], added to
  uint8_t* n_valid;        // optional, written once at the end
  uint8_t* piece;          // optional
  uint32_t* status;        // optional
  uint32_t B;
  uint32_t env_offset;     // global env index of env 0 (mod 2^32)
  int32_t P;
  int32_t n_steps;
  uint64_t seed;
  uint64_t step_idx0;
  tet::StepCfg cfg;        // (the keys are derived per step from seed and step_idx0)
  tet::SetTable tab;
};

struct SoftmaxRowsParams {
  const void* cols;
  const uint64_t* meta;
  const float* weights;    // as GreedyRowsParams
  const int32_t* rows;
  int32_t* action;
  float* logp;
  float* score;            // optional [B][8]
  float* logz;             // optional [B]
  float* logits;           // optional [B][a_max]
  uint32_t* status;        // optional
  int64_t B;
  int32_t P;
  int32_t R;
  int32_t a_max;
  int32_t has_direct_by;
  float direct_by[8];
  float inv_t;             // 1.0f / temperature
  uint32_t key;            // tet::softmax_key(seed, step_idx)
  uint32_t env_offset;     // global env index of env 0 (mod 2^32)
  tet::SetTable tab;
};

struct PlaySoftmaxParams {
  PlayParams play;         // as tetris_hip_play_linear (cfg carries direct_by)
  float* logp_total;       // optional [B], added to
  float* score_total;      // [B][8], added to
  float inv_t;
};

struct GatherParams {
  const void* src_cols;
  const uint64_t* src_meta;
  void* dst_cols;
  uint64_t* dst_meta;
  uint8_t* dst_n_valid;    // optional
  uint8_t* dst_piece;      // optional
  const int32_t* index;    // [B_dst]: src env, -1 = keep
  uint32_t* status;        // dst's per-wave counters or NULL
  int64_t B_src;
  int64_t B_dst;
  int32_t n_planes;
  uint64_t fullmask[tet::kMetaPieces];  // of the set's table (tet::SetTable); zero past the last piece
};

struct ExpandParams {
  const void* src_cols;
  const uint64_t* src_meta;
  void* dst_cols;
  uint64_t* dst_meta;
  const int32_t* parent;     // [B_dst]: src env, -1 = keep
  const int32_t* action;     // [B_dst]: placement of that env
  const uint8_t* next_piece; // [B_dst] list indices, or NULL: drawn from the parent's bag
  float* obs;                // optional [B_dst][8]
  int32_t* reward;
  uint8_t* done;
  uint8_t* lines;
  uint8_t* n_valid;
  uint8_t* piece;
  uint32_t* status;          // dst's per-wave counters or NULL
  uint32_t B_src;
  uint32_t B_dst;
  uint32_t env_offset;       // global env index of SRC env 0 (mod 2^32)
  tet::StepCfg cfg;          // auto_reset = 0; key_step is the step's
  tet::SetTable tab;
};

struct TwoPlyParams {
  const void* cols;
  const uint64_t* meta;
  float* values;             // optional [B][a_max][n_pieces]
  float* q;                  // optional [B][a_max]
  uint8_t* n_bag;            // optional [B]
  int32_t* best_action;      // optional [B]
  float* best_value;         // optional [B]
  int64_t B;
  int32_t R;
  int32_t a_max;
  int32_t n_pieces;
  float death_value;
  float w[8];
  tet::SetTable tab;
};

// the blocks travel as kernel arguments (4 KiB at the most), the table inside them
static_assert(sizeof(TwoPlyParams) <= 4096, "kernel argument block over 4 KiB");
static_assert(sizeof(StepManyParams) <= 4096 && sizeof(RolloutParams) <= 4096 && sizeof(AfterParams) <= 4096 &&
              sizeof(GreedyParams) <= 4096 && sizeof(ResetParams) <= 4096 && sizeof(GreedyRowsParams) <= 4096 &&
              sizeof(PlayParams) <= 4096 && sizeof(SoftmaxRowsParams) <= 4096 && sizeof(PlaySoftmaxParams) <= 4096 &&
              sizeof(ExpandParams) <= 4096,
              "kernel argument block over 4 KiB");

// bound step call: everything that does not change between steps is prepared once
struct TetrisStepCall {
  uint64_t magic;
  StepParams p{};
  TetrisDesc desc;
  uint64_t seed;
  int32_t* action_out;  // written only when the built-in policy draws the action
};
constexpr uint64_t kStepCallMagic = 0x5445545249535343ull;  // "TETRISSC"

}  // namespace

#ifndef __HIPCC__
// The CPU twin of gather_envs_kernel for a host build of this header (the CPU test harness): a loop over dst
// envs on the shared body, joining the launch overloads of the includer's backend (the unnamed namespaces of
// one translation unit are one namespace).  hipcc never sees it: the library has no CPU path.
namespace {
namespace backend {
template <typename W>
inline int gather_envs_host(const GatherParams& p) {
  const bool known = tet::gather_variant(p.n_planes, [&](auto np) {
    for (int64_t j = 0; j < p.B_dst; ++j) {
      const bool invalid = tet::gather_env<W, decltype(np)::value>(static_cast<const W*>(p.src_cols), p.src_meta, p.B_src,
                                                                  static_cast<W*>(p.dst_cols), p.dst_meta, p.dst_n_valid,
                                                                  p.dst_piece, p.index[j], j, p.fullmask);
      if (invalid && p.status) p.status[(j >> 6) * 4 + TETRIS_STATUS_INVALID] += 1;
    }
  });
  return known ? TETRIS_OK : TETRIS_E_COLUMNS;
}
inline int launch(const TetrisDesc* desc, const GatherParams& p, void*) {
  return desc->word_bytes == 4 ? gather_envs_host<uint32_t>(p) : gather_envs_host<uint64_t>(p);
}

// The CPU twins of greedy_rows_kernel and play_linear_kernel: loops over envs on the shared bodies
// (tet::greedy_pick_env, tet::play_step_env), on the instantiation the library launches for the geometry.
// f(W{}, IntConst<C>, IntConst<NCH>, IntConst<CR>, BoolConst<PACK>)
template <typename F>
inline int host_variant(const TetrisDesc* desc, F&& f) {
  switch (desc->num_columns) {
#define TET_X(CC)                                                                                                  \
  case CC:                                                                                                         \
    if (desc->word_bytes == 4)                                                                                     \
      tet::kernel_variant<uint32_t>(desc->num_rows, [&](auto nch, auto cr, auto pack) { f(uint32_t{}, tet::IntConst<CC>{}, nch, cr, pack); }); \
    else                                                                                                           \
      tet::kernel_variant<uint64_t>(desc->num_rows, [&](auto nch, auto cr, auto pack) { f(uint64_t{}, tet::IntConst<CC>{}, nch, cr, pack); }); \
    return TETRIS_OK;
    TET_COLUMNS(TET_X)
#undef TET_X
    default:
      return TETRIS_E_COLUMNS;
  }
}

template <typename W, int C, int NCH, bool PACK>
inline void greedy_rows_host(const GreedyRowsParams& p) {
  for (int64_t i = 0; i < p.B; ++i) {
    const int32_t row = p.rows ? p.rows[i] : (int32_t)i;
    if (!tet::weight_row_ok(row, p.P)) {  // untouched, counted
      if (p.status) p.status[(i >> 6) * 4 + TETRIS_STATUS_INVALID] += 1;
      continue;
    }
    float w[8];
    tet::load_weight_row(p.weights, row, w);
    W col[C];
    tet::load_board<W, C, PACK>(static_cast<const W*>(p.cols), p.B, i, col);
    const tet::GreedyPick pick = tet::greedy_pick_env<W, C, NCH>(col, p.meta[i], p.tab, kAfterLut.bytes, p.R, w);
    p.best_action[i] = pick.best_row;
    if (p.best_value) p.best_value[i] = pick.best;
  }
}
inline int launch(const TetrisDesc* desc, const GreedyRowsParams& p, void*) {
  return host_variant(desc, [&](auto w, auto c, auto nch, auto, auto pack) {
    greedy_rows_host<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(pack)::value>(p);
  });
}

template <typename W, int C, int NCH, bool PACK>
inline void play_linear_host(const PlayParams& p) {
  W* cols = static_cast<W*>(p.cols);
  const int64_t B = p.B;
  tet::StepCfg cfg = p.cfg;
  for (int64_t i = 0; i < B; ++i) {
    uint32_t* slot = p.status ? p.status + (i >> 6) * 4 : nullptr;
    const int32_t row = p.rows ? p.rows[i] : (int32_t)i;
    if (!tet::weight_row_ok(row, p.P)) {  // untouched, counted once per launch
      if (slot) slot[TETRIS_STATUS_INVALID] += 1;
      continue;
    }
    float w[8];
    tet::load_weight_row(p.weights, row, w);
    W col[C], scratch[C];
    tet::load_board<W, C, PACK>(cols, B, i, col);
    uint64_t m = p.meta[i];
    uint32_t lines = 0, pieces = 0;
    for (int k = 0; k < p.n_steps; ++k) {
      if (tet::env_over(m)) continue;  // frozen
      tet::step_keys(p.seed, p.step_idx0 + (uint64_t)k, cfg);
      tet::StepOut out;
      tet::play_step_env<W, C, NCH, false>(col, m, w, p.tab, kAfterLut.bytes, scratch, 1, cfg, p.env_offset + (uint32_t)i, out);
      if (out.invalid) continue;
      lines += (uint32_t)out.lines;
      pieces += 1;
      if (slot) {
        slot[TETRIS_STATUS_EPISODES] += out.done;
        slot[TETRIS_STATUS_LINES] += out.lines;
        slot[TETRIS_STATUS_STEPS] += 1;
      }
    }
    if (pieces) {
      tet::store_board<W, C, PACK>(cols, B, i, col);
      p.meta[i] = m;
      p.lines_total[i] += lines;
      p.pieces_total[i] += pieces;
    }
    if (p.n_valid) p.n_valid[i] = (uint8_t)tet::popc(tet::meta_mask(m));
    if (p.piece) p.piece[i] = (uint8_t)tet::meta_piece(m);
  }
}
inline int launch(const TetrisDesc* desc, const PlayParams& p, void*) {
  return host_variant(desc, [&](auto w, auto c, auto nch, auto, auto pack) {
    play_linear_host<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(pack)::value>(p);
  });
}

// The CPU twins of softmax_rows_kernel and play_softmax_kernel (tet::softmax_pick_env, tet::play_softmax_step_env);
// expf / logf are libm's here and the device library's there, so the two agree to rounding, not bit for bit.
template <typename W, int C, int NCH, bool PACK>
inline void softmax_rows_host(const SoftmaxRowsParams& p) {
  const float ninf = -__builtin_inff();
  for (int64_t i = 0; i < p.B; ++i) {
    const int32_t row = p.rows ? p.rows[i] : (int32_t)i;
    if (!tet::weight_row_ok(row, p.P)) {  // untouched, counted
      if (p.status) p.status[(i >> 6) * 4 + TETRIS_STATUS_INVALID] += 1;
      continue;
    }
    float w[8];
    tet::load_weight_row(p.weights, row, w);
    W col[C];
    tet::load_board<W, C, PACK>(static_cast<const W*>(p.cols), p.B, i, col);
    float* lrow = p.logits ? p.logits + i * (int64_t)p.a_max : nullptr;
    tet::SoftmaxPick pick;
    tet::softmax_pick_env<W, C, NCH>(col, p.meta[i], p.tab, kAfterLut.bytes, p.R, w, p.inv_t, p.has_direct_by != 0,
                                     p.direct_by, p.key, p.env_offset + (uint32_t)i, lrow, pick);
    if (lrow)
      for (int k = tet::popc(tet::meta_mask(p.meta[i]) & p.tab.fullmask[tet::meta_piece(p.meta[i])]); k < p.a_max; ++k) lrow[k] = ninf;
    p.action[i] = pick.action;
    p.logp[i] = pick.logp;
    if (p.logz) p.logz[i] = pick.logz;
    if (p.score)
      for (int q = 0; q < 8; ++q) p.score[i * 8 + q] = pick.score[q];
  }
}
inline int launch(const TetrisDesc* desc, const SoftmaxRowsParams& p, void*) {
  return host_variant(desc, [&](auto w, auto c, auto nch, auto, auto pack) {
    softmax_rows_host<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(pack)::value>(p);
  });
}

template <typename W, int C, int NCH, bool PACK>
inline void play_softmax_host(const PlaySoftmaxParams& q) {
  const PlayParams& p = q.play;
  W* cols = static_cast<W*>(p.cols);
  const int64_t B = p.B;
  tet::StepCfg cfg = p.cfg;
  for (int64_t i = 0; i < B; ++i) {
    uint32_t* slot = p.status ? p.status + (i >> 6) * 4 : nullptr;
    const int32_t row = p.rows ? p.rows[i] : (int32_t)i;
    if (!tet::weight_row_ok(row, p.P)) {  // untouched, counted once per launch
      if (slot) slot[TETRIS_STATUS_INVALID] += 1;
      continue;
    }
    float w[8];
    tet::load_weight_row(p.weights, row, w);
    W col[C], scratch[C];
    tet::load_board<W, C, PACK>(cols, B, i, col);
    uint64_t m = p.meta[i];
    uint32_t lines = 0, pieces = 0;
    float logp = q.logp_total ? q.logp_total[i] : 0.f, score[8];
    for (int j = 0; j < 8; ++j) score[j] = q.score_total[i * 8 + j];
    for (int k = 0; k < p.n_steps; ++k) {
      if (tet::env_over(m)) continue;  // frozen
      tet::step_keys(p.seed, p.step_idx0 + (uint64_t)k, cfg);
      tet::SoftmaxPick pick;
      tet::StepOut out;
      tet::play_softmax_step_env<W, C, NCH, false>(col, m, w, q.inv_t, tet::softmax_key(p.seed, p.step_idx0 + (uint64_t)k), p.tab,
                                                   kAfterLut.bytes, scratch, 1, cfg, p.env_offset + (uint32_t)i, pick, out);
      if (out.invalid) continue;
      lines += (uint32_t)out.lines;
      pieces += 1;
      logp = TET_FADD(logp, pick.logp);
      for (int j = 0; j < 8; ++j) score[j] = TET_FADD(score[j], pick.score[j]);
      if (slot) {
        slot[TETRIS_STATUS_EPISODES] += out.done;
        slot[TETRIS_STATUS_LINES] += out.lines;
        slot[TETRIS_STATUS_STEPS] += 1;
      }
    }
    if (pieces) {
      tet::store_board<W, C, PACK>(cols, B, i, col);
      p.meta[i] = m;
      p.lines_total[i] += lines;
      p.pieces_total[i] += pieces;
      if (q.logp_total) q.logp_total[i] = logp;
      for (int j = 0; j < 8; ++j) q.score_total[i * 8 + j] = score[j];
    }
    if (p.n_valid) p.n_valid[i] = (uint8_t)tet::popc(tet::meta_mask(m));
    if (p.piece) p.piece[i] = (uint8_t)tet::meta_piece(m);
  }
}
inline int launch(const TetrisDesc* desc, const PlaySoftmaxParams& p, void*) {
  return host_variant(desc, [&](auto w, auto c, auto nch, auto, auto pack) {
    play_softmax_host<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(pack)::value>(p);
  });
}

// The CPU twin of expand_kernel: a loop over dst envs on tet::expand_entry / tet::expand_env, on the instantiation and
// the feature tables step_kernel runs for the geometry.
template <typename W, int C, int NCH, int CR, bool PACK>
inline void expand_host(const ExpandParams& p) {
  const uint8_t* lut = CR == 10 ? kFeatureLut10.bytes : kFeatureLut.bytes;
  for (int64_t j = 0; j < (int64_t)p.B_dst; ++j) {
    const int32_t parent = p.parent[j];
    const int np = p.next_piece ? (int)p.next_piece[j] : -1;
    const int entry = tet::expand_entry(parent, p.B_src, np, p.cfg.n_pieces);
    if (entry == tet::kExpandKeep) continue;
    bool bad = entry == tet::kExpandBad;
    W col[C], scratch[C];
    uint64_t m = 0;
    tet::StepOut out;
    if (!bad) {
      tet::load_board<W, C, PACK>(static_cast<const W*>(p.src_cols), p.B_src, parent, col);
      m = p.src_meta[parent];
      tet::expand_env<W, C, NCH, CR, false>(col, m, p.action[j], np, p.tab, lut, scratch, 1, p.cfg, p.env_offset + (uint32_t)parent, out);
      bad = out.invalid != 0;
    }
    if (bad) {  // untouched, counted
      if (p.status) p.status[(j >> 6) * 4 + TETRIS_STATUS_INVALID] += 1;
      continue;
    }
    tet::store_board<W, C, PACK>(static_cast<W*>(p.dst_cols), p.B_dst, j, col);
    p.dst_meta[j] = m;
    if (p.obs)
      for (int k = 0; k < 8; ++k) p.obs[j * 8 + k] = out.obs[k];
    p.reward[j] = out.reward;
    p.done[j] = (uint8_t)out.done;
    p.lines[j] = (uint8_t)out.lines;
    p.n_valid[j] = (uint8_t)out.n_valid;
    p.piece[j] = (uint8_t)out.piece;
  }
}
inline int launch(const TetrisDesc* desc, const ExpandParams& p, void*) {
  return host_variant(desc, [&](auto w, auto c, auto nch, auto cr, auto pack) {
    expand_host<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(cr)::value, decltype(pack)::value>(p);
  });
}

// The CPU twin of two_ply_kernel: a loop over envs and first actions on tet::two_ply_lane, then tet::two_ply_pick over
// the env's row of sums -- the same ascending-p additions and the same walk as the kernel's.
template <typename W, int C, int NCH, bool PACK>
inline void two_ply_host(const TwoPlyParams& p) {
  float q_row[4 * tet::kMaxCols];  // a_max <= 48: the placements one valid mask holds
  for (int64_t i = 0; i < p.B; ++i) {
    W col0[C];
    tet::load_board<W, C, PACK>(static_cast<const W*>(p.cols), p.B, i, col0);
    const uint64_t m = p.meta[i];
    const uint32_t bag = tet::two_ply_bag(m, p.n_pieces);
    for (int k = 0; k < p.a_max; ++k) {
      W col[C], scratch[C];
      for (int c = 0; c < C; ++c) col[c] = col0[c];
      float* row = p.values ? p.values + (i * p.a_max + k) * (int64_t)p.n_pieces : nullptr;
      q_row[k] = tet::two_ply_lane<W, C, NCH, false>(col, m, k, bag, p.w, p.death_value, p.n_pieces, p.tab, kAfterLut.bytes,
                                                     scratch, 1, p.R, row);
      if (p.q) p.q[i * p.a_max + k] = q_row[k];
    }
    const tet::GreedyPick pick = tet::two_ply_pick(q_row, tet::two_ply_n_valid(m, p.a_max));
    if (p.n_bag) p.n_bag[i] = (uint8_t)tet::popc(bag);
    if (p.best_action) p.best_action[i] = pick.best_row;
    if (p.best_value) p.best_value[i] = pick.best;
  }
}
inline int launch(const TetrisDesc* desc, const TwoPlyParams& p, void*) {
  return host_variant(desc, [&](auto w, auto c, auto nch, auto, auto pack) {
    two_ply_host<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(pack)::value>(p);
  });
}
}  // namespace backend
}  // namespace
#endif
