// core_host.cpp -- TEST HARNESS ONLY: compiles the per-lane device logic of
// tetris_amd/csrc/tetris_core.hpp for the host (g++) so that the CPU test
// suite (and -fsanitize builds) can check it against the oracle without a GPU.
// It is not part of the product: nothing under tetris_amd/ loads it, and the
// product path (libtetris_hip.so) has no CPU fallback.
//
// The C-ABI is the library's own text (tetris_amd/csrc/tetris_abi.inc: checks, keys, parameter blocks, the
// bound step call) under the tetris_host_ prefix; this file is the backend it runs on.  Each *_impl is the
// CPU twin of the kernel that takes the same parameter block in tetris_kernels.hip, looping over envs instead
// of lanes: it runs the template instantiation the library would launch for the same TetrisDesc
// (tet::kernel_variant) on the tables the kernel stages, and calls the same per-env bodies (tetris_core.hpp,
// tetris_entry.hpp); only what a GPU alone needs is missing.
#include <stdint.h>
#include <string.h>

#include "../../include/tetris_hip.h"
#include "../../tetris_amd/csrc/tetris_entry.hpp"

namespace {

// the feature tables a stepping kernel of chunk size CR stages
template <int CR>
const uint8_t* step_lut() { return CR == 10 ? kFeatureLut10.bytes : kFeatureLut.bytes; }

// one slot of 4 counters per 64 envs (= per wavefront on the GPU)
void count_status(uint32_t* status, int64_t i, const tet::StepOut& out) {
  if (!status) return;
  uint32_t* slot = status + (i >> 6) * 4;
  slot[TETRIS_STATUS_INVALID] += out.invalid;
  if (!out.invalid) {
    slot[TETRIS_STATUS_EPISODES] += out.done;
    slot[TETRIS_STATUS_LINES] += out.lines;
    slot[TETRIS_STATUS_STEPS] += 1;
  }
}

// 64 envs at a time, as one wavefront of the kernel: one counter slot, one word of the done mask
template <typename W, int C, int NCH, int CR, bool PACK>
void step_impl(const StepParams& p) {
  tet::StepCfg cfg = p.cfg;
  if (p.step_counter) tet::step_keys(p.seed, *p.step_counter + p.step_rel, cfg);  // as the kernel: the counter's keys
  W* cols = static_cast<W*>(p.cols);
  const int64_t B = p.B;
  for (int64_t g = 0; g < B; g += 64) {
    uint32_t slot[4] = {0, 0, 0, 0};
    if (p.status) memcpy(slot, p.status + (g >> 6) * 4, sizeof slot);
    unsigned long long done_mask = 0;
    for (int64_t i = g; i < B && i < g + 64; ++i) {
      W col[C];
      tet::load_board<W, C, PACK>(cols, B, i, col);
      uint64_t m = p.meta[i];
      int draw, draw_reset, cur;
      bool exhausted;
      tet::stream_read(p.stream, p.cursor, p.stream_len, B, i, cfg, draw, draw_reset, cur, exhausted);
      tet::StepOut out;
      W scratch[C];
      tet::env_step<W, C, NCH, CR>(col, m, (p.action && !exhausted) ? p.action[i] : -1, p.action == nullptr && !exhausted,
                                   p.tab, step_lut<CR>(), scratch, 1, cfg, p.env_offset + (uint32_t)i, draw, draw_reset, out);
      if (p.action_out) p.action_out[i] = out.action;
      if (!out.invalid) {
        tet::store_board<W, C, PACK>(cols, B, i, col);
        p.meta[i] = m;
        if (p.stream) p.cursor[i] = tet::stream_advance(cur, out, cfg);
      }
      if (p.obs)
        for (int k = 0; k < 8; ++k) p.obs[i * 8 + k] = out.obs[k];
      p.reward[i] = out.reward;
      p.done[i] = (uint8_t)out.done;
      p.lines[i] = (uint8_t)out.lines;
      p.n_valid[i] = (uint8_t)out.n_valid;
      if (p.piece_next) p.piece_next[i] = (uint8_t)out.piece;
      count_status(slot, 0, out);
      done_mask |= (unsigned long long)(out.done != 0) << (i & 63);
    }
    if (p.status) memcpy(p.status + (g >> 6) * 4, slot, sizeof slot);
    if (p.status || p.done_bits) {  // the gather payload: this step's done mask, the counters as of this step
      if (p.status_snapshot) memcpy(p.status_snapshot + (g >> 6) * 4, slot, sizeof slot);
      if (p.done_bits) p.done_bits[g >> 6] = done_mask;
    }
  }
}

template <typename W, int C, int NCH, int CR, bool PACK>
void step_many_impl(const StepManyParams& q) {
  const StepParams& p = q.one;
  tet::StepCfg cfg = p.cfg;
  W* cols = static_cast<W*>(p.cols);
  const int64_t B = p.B;
  for (int64_t i = 0; i < B; ++i) {
    W col[C];
    tet::load_board<W, C, PACK>(cols, B, i, col);
    uint64_t m = p.meta[i];
    for (int k = 0; k < q.n_steps; ++k) {
      tet::step_keys(q.seed, q.step_idx0 + k, cfg);
      W scratch[C];
      tet::StepOut out;
      if (q.policy == 1) {  // as the kernel: the greedy variant picks and steps on the afterstate tables, 12-row chunks
        tet::GreedyPick pick;
        tet::afterstates_env<W, C, NCH>(col, m, p.tab, kAfterLut.bytes, cfg.R, [&](bool has, int, int, float (&f)[8], int, int row, bool is_valid) {
          if (has && is_valid) pick.offer(tet::fitness_of(f, q.w), row);
        });
        tet::env_step<W, C, NCH, 12, true>(col, m, pick.best_row, false, p.tab, kAfterLut.bytes, scratch, 1, cfg,
                                           p.env_offset + (uint32_t)i, -1, -1, out);
      } else
        tet::env_step<W, C, NCH, CR>(col, m, -1, true, p.tab, step_lut<CR>(), scratch, 1, cfg, p.env_offset + (uint32_t)i,
                                     -1, -1, out);
      const int64_t e = (int64_t)k * B + i;
      if (p.obs)
        for (int j = 0; j < 8; ++j) p.obs[e * 8 + j] = out.obs[j];
      p.reward[e] = out.reward;
      p.done[e] = (uint8_t)out.done;
      p.lines[e] = (uint8_t)out.lines;
      p.n_valid[e] = (uint8_t)out.n_valid;
      if (p.piece_next) p.piece_next[e] = (uint8_t)out.piece;
      if (p.action_out) p.action_out[e] = out.action;
      count_status(p.status, i, out);
    }
    tet::store_board<W, C, PACK>(cols, B, i, col);
    p.meta[i] = m;
  }
}

template <typename W, int C, bool PACK>
void reset_impl(const ResetParams& p) {
  for (int64_t i = 0; i < p.B; ++i) {
    if (p.reset_mask && !p.reset_mask[i]) continue;
    const int cur = p.stream ? p.cursor[i] : 0;
    if (p.stream && tet::stream_reset_exhausted(cur, p.stream_len)) {  // untouched, counted
      if (p.status) p.status[(i >> 6) * 4 + TETRIS_STATUS_INVALID] += 1;
      continue;
    }
    tet::reset_env<W, C, PACK>(static_cast<W*>(p.cols), p.meta, p.B, i, p.tab, p.init_bag, p.n_pieces, p.key, p.env_offset,
                               p.stream, p.cursor, cur, p.piece_out, p.n_valid_out);
  }
}

template <typename W, int C, int NCH, bool PACK>
void after_impl(const AfterParams& p) {
  const tet::SetTable& tab = p.tab;
  const W* cols = static_cast<const W*>(p.cols);
  const int64_t rs = p.row_stride;
  for (int64_t i = 0; i < p.B; ++i) {
    W col[C];
    int h[C];
    tet::load_board<W, C, PACK>(cols, p.B, i, col);
    tet::heights_of<W, C>(col, h);
    const uint64_t meta = p.meta[i];
    const int piece = tet::meta_piece(meta);
    const uint64_t full = tab.fullmask[piece];
    const uint64_t valid = tet::meta_mask(meta) & full;
    float* out_valid = p.feats + i * p.env_stride;
    float* out_all = p.feats_all ? p.feats_all + i * p.env_stride : nullptr;
    for (int k = 0; k < p.a_max; ++k) {
      memset(out_valid + k * rs, 0, sizeof(float) * 8);
      if (out_all) memset(out_all + k * rs, 0, sizeof(float) * 8);
    }
    int nv = tet::popc(valid), na = tet::popc(full);
    bool consistent = true;
    tet::afterstates_env<W, C, NCH>(col, meta, tab, kAfterLut.bytes, p.R, [&](bool has, int sk, int sc, float (&f)[8], int row_all, int row_valid, bool is_valid) {
      if (!has) return;
      const int s = tet::mask_bit(sk, sc);
      // (0) the running row indices of the walk against the popcount form
      consistent = consistent && row_all == tet::row_of_slot<C>(full, sk, sc) && is_valid == (bool)((valid >> s) & 1) &&
                   (!is_valid || row_valid == tet::row_of_slot<C>(valid, sk, sc));
      // cross-checks (test harness only): (1) the incremental features against the full
      // evaluation of the same placement, (2) the cached mask against the direct terminal test
      const tet::Orient o = tet::unpack_orient(tab.orient[piece][sk].desc);
      W nb[C];
      W pbits[4];
      int nh[C];
      const int a = tet::stamp_static<W, C>(col, h, sc, o, nb, pbits);
      int eroded = 0;
      const int k = tet::clear_lines<W, C>(nb, pbits, a, &eroded);
      tet::heights_of<W, C>(nb, nh);
      float g[8];
      tet::bcts_features<W, C>(nb, nh, p.R, kFeatureLut.bytes, a, o.H, eroded, k, g);
      for (int q = 0; q < 8; ++q) consistent = consistent && (g[q] == f[q]);
      const bool terminal = (a + o.H - k) > p.R;  // state.py:36 after :33
      consistent = consistent && (terminal != (bool)((valid >> s) & 1));
      if (p.has_direct_by)
        for (int q = 0; q < 8; ++q) f[q] *= p.direct_by[q];
      if (out_all) memcpy(out_all + tet::row_of_slot<C>(full, sk, sc) * rs, f, sizeof(float) * 8);
      if ((valid >> s) & 1) memcpy(out_valid + tet::row_of_slot<C>(valid, sk, sc) * rs, f, sizeof(float) * 8);
    });
    if (!consistent) nv = 255;  // fail loudly in the tests
    p.n_valid[i] = (uint8_t)nv;
    if (p.n_all) p.n_all[i] = (uint8_t)na;
  }
}

template <typename W, int C, int NCH, bool PACK>
void greedy_impl(const GreedyParams& p) {
  const W* cols = static_cast<const W*>(p.cols);
  for (int64_t i = 0; i < p.B; ++i) {
    W col[C];
    tet::load_board<W, C, PACK>(cols, p.B, i, col);
    const uint64_t full = p.tab.fullmask[tet::meta_piece(p.meta[i])];
    float* fall = p.fitness_all ? p.fitness_all + i * p.a_max : nullptr;
    if (fall)
      for (int k = 0; k < p.a_max; ++k) fall[k] = 0.f;
    tet::GreedyPick pick;
    tet::afterstates_env<W, C, NCH>(col, p.meta[i], p.tab, kAfterLut.bytes, p.R, [&](bool has, int sk, int sc, float (&f)[8], int, int row, bool is_valid) {
      if (!has) return;
      const float v = tet::fitness_of(f, p.w);
      if (fall) fall[tet::row_of_slot<C>(full, sk, sc)] = v;
      if (is_valid) pick.offer(v, row);
    });
    p.best_action[i] = pick.best_row;
    if (p.best_value) p.best_value[i] = pick.best;
  }
}

template <typename W, int C, int NCH, bool PACK>
void rollouts_impl(const RolloutParams& p) {
  const W* cols = static_cast<const W*>(p.cols);
  for (int64_t i = 0; i < p.B; ++i) {
    W col[C], scratch[C];
    tet::load_board<W, C, PACK>(cols, p.B, i, col);
    for (int a0 = 0; a0 < p.a_max; ++a0)
      p.returns[i * p.a_max + a0] = tet::rollout_mean<W, C, NCH>(col, p.meta[i], i, a0, p.env_offset, p.a_max, p.n, p.length,
                                                                 p.policy, p.w, p.tab, kAfterLut.bytes, scratch, 1, p.R,
                                                                 p.n_pieces, p.key, p.pieces);
  }
}

template <typename W>
void decode_impl(const W* cols, int8_t* cells, int32_t* heights, int C, int rows, int64_t B, bool packed) {
  for (int64_t i = 0; i < B; ++i)
    for (int c = 0; c < C; ++c) {
      const W x = tet::load_column_rt<W>(cols, B, i, c, C, packed);
      if (heights) heights[i * C + c] = tet::bitlen(x);
      if (cells)
        for (int r = 0; r < rows; ++r) cells[(i * rows + r) * C + c] = (int8_t)((x >> r) & 1);
    }
}

template <typename W>
void encode_impl(const int8_t* cells, W* cols, int C, int rows, int64_t B, bool packed) {
  for (int64_t i = 0; i < B; ++i) {
    W col[tet::kMaxCols];
    for (int c = 0; c < C; ++c) {
      W x = 0;
      for (int r = 0; r < rows; ++r) x |= (W)(cells[(i * rows + r) * C + c] != 0) << r;
      col[c] = x;
    }
    tet::store_columns_rt<W>(cols, B, i, col, C, packed);
  }
}

// the harness's launch: f(W{}, IntConst<C>, IntConst<NCH>, IntConst<CR>, BoolConst<PACK>) on the word and column
// count of the descriptor and the variant the library's launchers pick for it
template <typename W, int C, typename F>
void with_variant(int R, F& f) {
  tet::kernel_variant<W>(R, [&](auto nch, auto cr, auto pack) { f(W{}, tet::IntConst<C>{}, nch, cr, pack); });
}
template <typename F>
int dispatch(const TetrisDesc* desc, F&& f) {
  switch (desc->num_columns) {
#define TET_X(CC)                                                      \
  case CC:                                                             \
    if (desc->word_bytes == 4) with_variant<uint32_t, CC>(desc->num_rows, f); \
    else with_variant<uint64_t, CC>(desc->num_rows, f);                \
    return 0;
    TET_COLUMNS(TET_X)
#undef TET_X
    default:
      return TETRIS_E_COLUMNS;
  }
}

namespace backend {

constexpr const char* kSourceHash = "harness";
const char* error_text(int) { return "unknown error"; }

int launch(const TetrisDesc* d, const StepParams& p, void*) {
  return dispatch(d, [&](auto w, auto c, auto nch, auto cr, auto pack) {
    step_impl<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(cr)::value, decltype(pack)::value>(p);
  });
}
int launch(const TetrisDesc* d, const StepManyParams& p, void*) {
  return dispatch(d, [&](auto w, auto c, auto nch, auto cr, auto pack) {
    step_many_impl<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(cr)::value, decltype(pack)::value>(p);
  });
}
int launch(const TetrisDesc* d, const ResetParams& p, void*) {
  return dispatch(d, [&](auto w, auto c, auto, auto, auto pack) { reset_impl<decltype(w), decltype(c)::value, decltype(pack)::value>(p); });
}
int launch(const TetrisDesc* d, const RefreshParams& p, void*) {
  return dispatch(d, [&](auto w, auto c, auto, auto, auto pack) {
    for (int64_t i = 0; i < p.B; ++i)
      tet::refresh_env<decltype(w), decltype(c)::value, decltype(pack)::value>(static_cast<const decltype(w)*>(p.cols), p.meta,
                                                                            p.n_valid_out, p.B, i, p.tab, p.R);
  });
}
int launch(const TetrisDesc* d, const AfterParams& p, void*) {
  return dispatch(d, [&](auto w, auto c, auto nch, auto, auto pack) {
    after_impl<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(pack)::value>(p);
  });
}
int launch(const TetrisDesc* d, const GreedyParams& p, void*) {
  return dispatch(d, [&](auto w, auto c, auto nch, auto, auto pack) {
    greedy_impl<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(pack)::value>(p);
  });
}
int launch(const TetrisDesc* d, const RolloutParams& p, void*) {
  return dispatch(d, [&](auto w, auto c, auto nch, auto, auto pack) {
    rollouts_impl<decltype(w), decltype(c)::value, decltype(nch)::value, decltype(pack)::value>(p);
  });
}

int stream_link(void*, void*) { return 0; }
int pack_done_bits(const uint8_t* done, uint8_t* bits, int64_t B, void*) {  // whole 64-bit words, as the kernel's ballots
  memset(bits, 0, (size_t)((B + 63) / 64) * 8);
  for (int64_t i = 0; i < B; ++i)
    if (done[i]) bits[i >> 3] |= (uint8_t)(1u << (i & 7));
  return 0;
}
int counter_add(uint64_t* counter, uint64_t n, void*) {
  *counter += n;
  return 0;
}
int policy_random(const uint8_t* n_valid, int32_t* action, uint32_t key, int64_t env_offset, int64_t B, void*) {
  for (int64_t i = 0; i < B; ++i) action[i] = tet::policy_random(key, (uint32_t)(env_offset + i), n_valid[i]);
  return 0;
}
int numpy_bag_stream(const uint32_t* seeds, int32_t n_pieces, int64_t L, uint8_t* stream, int64_t B, void*) {
  for (int64_t i = 0; i < B; ++i) tet::numpy_bag_stream_env(seeds, n_pieces, L, stream, B, i);
  return 0;
}
int decode(int word_bytes, const void* cols, int8_t* cells, int32_t* heights, int C, int rows, int64_t B, bool packed, void*) {
  if (word_bytes == 4) decode_impl(static_cast<const uint32_t*>(cols), cells, heights, C, rows, B, packed);
  else decode_impl(static_cast<const uint64_t*>(cols), cells, heights, C, rows, B, packed);
  return 0;
}
int encode(int word_bytes, const int8_t* cells, void* cols, int C, int rows, int64_t B, bool packed, void*) {
  if (word_bytes == 4) encode_impl(cells, static_cast<uint32_t*>(cols), C, rows, B, packed);
  else encode_impl(cells, static_cast<uint64_t*>(cols), C, rows, B, packed);
  return 0;
}

}  // namespace backend
}  // namespace

#define TET_ABI(name) tetris_host_##name
#include "../../tetris_amd/csrc/tetris_abi.inc"
