// tetris_kernels.hip -- gfx950 kernels + the C-ABI of include/tetris_hip.h (its text: tetris_abi.inc).
//
// One lane per env; column bitboards in tile-major HBM storage (tet::plane_index: the planes of a
// wavefront's 64 envs back to back, one contiguous record per wave; 256 contiguous bytes (u32) or 512
// (u64) per plane and wave).  No dense contraction anywhere -> no MFMA; the path is integer bit work
// (popcount / clz / shifts / byte-table reads from LDS) over state streamed from HBM, and it is bound by
// vector-instruction issue, not by bytes.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tetris_hip.h"
#include "tetris_entry.hpp"

namespace {

using tet::SetTable;
using tet::StepCfg;

constexpr int kBlock = 256;

// minimum waves per SIMD the step kernel is compiled for (bounds its VGPR budget).  u32 boards: 5
// -- the kernel needs 73 VGPRs (80 allocated: 6 waves per SIMD = three 512-env workgroups per CU),
// no spills.  u64 boards: 103-129 VGPRs (4 / 3 waves per SIMD).  Builds with 7 and 8 waves per SIMD
// (256-env tiles at 71 VGPRs; 512-env tiles squeezed to 64) were timed in round 2 and are not
// faster: profiles/r02_experiments/sweep_compacted_mask_and_occupancy_variants.txt.
#ifndef TET_STEP_WAVES
#define TET_STEP_WAVES 0
#endif
template <typename W, int CR = 12>
constexpr int step_waves() { return TET_STEP_WAVES ? TET_STEP_WAVES : (sizeof(W) == 4 ? 5 : (CR == 10 ? 4 : 3)); }

// envs per workgroup of the step kernel: the feature tables are staged once per workgroup, so a
// larger tile amortises that L2 -> LDS traffic over more envs.  u32 boards: 512 (8 waves = 2 per
// SIMD per workgroup, three workgroups per CU; 320, 640 and 1024 are slower: uneven waves per
// SIMD / one workgroup per CU; 256 is within 1 %).  u64 boards keep 256 (their registers allow
// 3-4 waves per SIMD = three or four 256-env workgroups).
#ifndef TET_STEP_BLOCK
#define TET_STEP_BLOCK 0
#endif
template <typename W>
constexpr int step_block() { return TET_STEP_BLOCK ? TET_STEP_BLOCK : (sizeof(W) == 4 ? 512 : 256); }

// Diagnostic build only (-DTET_STAMPS=1, tools/timeline.py): every workgroup of the step kernel
// records when it started, when its loads had landed, when it began to store and when it ended
// (s_memrealtime, 100 MHz) plus where it ran.  Never compiled into the product library.
#ifndef TET_STAMPS
#define TET_STAMPS 0
#endif
#if TET_STAMPS
constexpr int kStampWgs = 16384, kStampWords = 20;  // (slots 6.. are per-tile stamps of looping variants; unused here)
__device__ uint64_t g_stamps[kStampWgs * kStampWords];
#define TET_STAMP(slot) do { if (threadIdx.x == 0 && blockIdx.x < kStampWgs) g_stamps[blockIdx.x * kStampWords + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define TET_STAMP(slot) ((void)0)
#endif

// ---- kernels ------------------------------------------------------------------

// the table blobs (kFeatureLut, kFeatureLut10, kAfterLut: tetris_entry.hpp) are copied to LDS as one block each
static_assert(tet::kAfterLutBytes % 16 == 0, "staged as uint4");
template <int CR>
__device__ __forceinline__ const uint4* feature_lut_src() {
  return CR == 10 ? reinterpret_cast<const uint4*>(&kFeatureLut10) : reinterpret_cast<const uint4*>(&kFeatureLut);
}
__device__ __forceinline__ void stage_after_lut(uint8_t* lds) {
  const uint4* src = reinterpret_cast<const uint4*>(&kAfterLut);
  uint4* dst = reinterpret_cast<uint4*>(lds);
  for (int t = threadIdx.x; t < tet::kAfterLutBytes / 16; t += blockDim.x) dst[t] = src[t];
}

// Everything a stepping workgroup keeps in LDS, as ONE object so that the placement table sits at
// LDS address 0: its reads then fit the 8-bit offsets of ds_read2 / the offset field of
// ds_read_b128 and need no per-read address arithmetic.
template <typename W, int C, int BLK, int CR, bool AFTER = false>
struct alignas(16) StepLds {
  SetTable tab;
  // AFTER: a tet::AfterLut; else the tables at their own offsets, up to the last byte this geometry's kernels read
  // (NCH = 2 is the only chunk count 32-bit boards run with the 10-row tables)
  alignas(16) uint8_t lut[AFTER ? tet::kAfterLutBytes
                                : (tet::features_packed<W, C, 2, CR>() ? tet::LutLayout<CR>::kBytes : tet::LutLayout<CR>::kByteTablesEnd)];
  // per-lane scratch for the runtime-indexed stamp (bank = lane); C + 3 columns where tet::stamp_scratch runs unclamped
  W lane_cols[tet::scratch_cols<W, C, 2, CR, AFTER>()][BLK];
};

// The part of the feature tables a stepping kernel reads, in 16-byte units [begin, end): the byte tables and
// the select tables, or -- where tet::board_features_u32_2x10 runs -- the select tables and the packed entries
// behind them.  LDS holds the whole block at its own offsets either way; the rest is never touched.
template <typename W, int C, int NCH, int CR>
constexpr int lut_stage_begin() { return tet::features_packed<W, C, NCH, CR>() ? tet::LutLayout<CR>::kSelPair / 16 : 0; }
template <typename W, int C, int NCH, int CR>
constexpr int lut_stage_end() {
  return (tet::features_packed<W, C, NCH, CR>() ? tet::LutLayout<CR>::kBytes : tet::LutLayout<CR>::kByteTablesEnd) / 16;
}
static_assert(tet::LutLayout<10>::kSelPair % 16 == 0 && tet::LutLayout<10>::kByteTablesEnd % 16 == 0 && tet::LutLayout<10>::kBytes % 16 == 0, "staged as uint4");

template <typename W, int C, int NCH, int CR>
__device__ __forceinline__ void stage_hole_lut(uint8_t* lds) {
  const uint4* src = feature_lut_src<CR>();
  uint4* dst = reinterpret_cast<uint4*>(lds);
  for (int t = lut_stage_begin<W, C, NCH, CR>() + (int)threadIdx.x; t < lut_stage_end<W, C, NCH, CR>(); t += blockDim.x) dst[t] = src[t];
}

__device__ __forceinline__ void stage_table(SetTable& lds, const SetTable& arg) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&arg);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&lds);
  for (int t = threadIdx.x; t < (int)(sizeof(SetTable) / 4); t += blockDim.x) dst[t] = src[t];
  __syncthreads();
}

// Per-wave counters without atomics: same-address atomics from 16k waves serialise
// at ~12 ns each (measured: 430 us per launch), so every wave owns one 16-byte slot
// of `status` and lane 0 read-modify-writes it (launches are stream-ordered).
__device__ __forceinline__ unsigned wave_sum(int value_bits, int v) {
  unsigned total = 0;
  for (int b = 0; b < value_bits; ++b) {
    unsigned long long m = __ballot((v >> b) & 1);
    total += (unsigned)__popcll(m) << b;
  }
  return total;
}
// number of lanes of the wave for which `cond` holds: the comparison result feeds the ballot as it is
// (no 0 / 1 integer is built per lane and tested again)
__device__ __forceinline__ unsigned wave_count(bool cond) { return (unsigned)__popcll(__ballot(cond)); }

// Access element `byte_off / sizeof(T)` of a wave-uniform array through a 32-bit BYTE offset:
// base stays in SGPRs and the lane offset is one shared VGPR (global_load/store saddr form)
// instead of a 64-bit VGPR address per access.  Callers guarantee byte_off < 2^32.
template <typename T>
__device__ __forceinline__ T ld_off(const T* base, uint32_t byte_off) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}
template <typename T>
__device__ __forceinline__ void st_off(T* base, uint32_t byte_off, T v) {
  *reinterpret_cast<T*>(reinterpret_cast<char*>(base) + byte_off) = v;
}

// The board of env i goes back to its planes (packed storage: tet::pack_board).
// byte offset of (env i, plane 0) in the tile-major storage: < 2^32 for every batch the C-ABI accepts
template <typename W, int NP>
__device__ __forceinline__ uint32_t record_off(uint32_t i) {
  return ((i >> 6) * (uint32_t)(NP * 64) + (i & 63u)) * (uint32_t)sizeof(W);
}
template <typename W, int C, bool PACK>
__device__ __forceinline__ void store_planes(const StepParams& p, uint32_t i, const W (&col)[C]) {
  constexpr int NP = tet::n_planes(C, PACK);
  W w[NP];
  tet::pack_board<W, C, PACK>(col, w);
  const uint32_t off = record_off<W, NP>(i);
#pragma unroll
  for (int q = 0; q < NP; ++q) st_off(static_cast<W*>(p.cols), off + (uint32_t)(q * 64 * sizeof(W)), w[q]);
}

// Everything one lane reads for one env.
template <typename W, int C>
struct StepInputs {
  W col[C];
  uint64_t meta;
  int action;
  int draw, draw_reset, cursor;
  bool exhausted;  // replay stream: this step could run past the last recorded row
  uint4 status;
};

template <typename W, int C, bool PACK>
__device__ __forceinline__ void load_inputs(const StepParams& p, uint32_t i, StepInputs<W, C>& in) {
  const uint32_t ii = i < p.B ? i : 0;
  constexpr int NP = tet::n_planes(C, PACK);
  W w[NP];
  const uint32_t off = record_off<W, NP>(ii);
#pragma unroll
  for (int q = 0; q < NP; ++q) w[q] = ld_off(static_cast<const W*>(p.cols), off + (uint32_t)(q * 64 * sizeof(W)));
  tet::unpack_board<W, C, PACK>(w, in.col);
  in.meta = ld_off(p.meta, ii * 8u);
  in.action = p.action ? ld_off(p.action, ii * 4u) : -1;
  tet::stream_read(p.stream, p.cursor, p.stream_len, p.B, ii, p.cfg, in.draw, in.draw_reset, in.cursor, in.exhausted);
  in.status = make_uint4(0, 0, 0, 0);
  if (p.status) in.status = ld_off(reinterpret_cast<const uint4*>(p.status), (i >> 6) * 16u);  // this wave's slot
}

// One tile of envs per workgroup.  Persistent variants were measured in both rounds and are not
// faster: round 1's grid-stride loops (register prefetch, or 2 / 4 / 8 tiles per workgroup) were
// 3-20 % slower; round 2's per-wavefront loop with LDS-DMA prefetch of the next tile (no load is
// ever waited for, tables staged once per launch) ties at 1 Mi envs and loses elsewhere -- the SIMD
// arbitrates by age, so the oldest waves race ahead and the youngest finish the launch alone;
// evening that out with s_setprio recovers the tie, no more (profiles/r02_experiments/).
// NCH = number of 12-row chunks of the stored board, fixed at compile time for the common
// geometries (2: up to 24 stored rows, e.g. 10x20; 4: up to 48, e.g. 10x40), 0 = decide from R.
// BLK: envs per workgroup (step_block<W>(), or 256 for the small-batch variant of the headline geometry).
template <typename W, int C, int NCH, int CR, int BLK = step_block<W>()>
__global__ __launch_bounds__(BLK, (step_waves<W, CR>())) void step_kernel(const StepParams p) {
  constexpr int kBlock = BLK;  // shadows the file-wide tile size inside this kernel
  __shared__ StepLds<W, C, kBlock, CR> lds;
  SetTable& tab = lds.tab;
  uint8_t* const hole_lut = lds.lut;
  auto& lane_cols = lds.lane_cols;
  static_assert(sizeof(lds.lane_cols) / sizeof(lds.lane_cols[0]) >= (tet::scratch_padded<W, C, NCH, CR, false>() ? C + 3 : C), "the unclamped stamp needs its three columns");
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < p.B;
  // Issue every global load of this lane first (board, meta, action, counters, its share of the
  // two tables) so that one memory latency covers them all; only then fill LDS and barrier.
  constexpr bool PACK = NCH != 0 && !TET_NO_PACK;  // the launchers pick a counted-chunk variant exactly for packed boards
  TET_STAMP(0);
  StepInputs<W, C> in;
  load_inputs<W, C, PACK>(p, i, in);
  {
    constexpr int kLutVec0 = lut_stage_begin<W, C, NCH, CR>();
    constexpr int kLutVecs = lut_stage_end<W, C, NCH, CR>() - kLutVec0, kLutPerLane = (kLutVecs + kBlock - 1) / kBlock;
    const uint4* lsrc = feature_lut_src<CR>() + kLutVec0;
    uint4 lv[kLutPerLane];
#pragma unroll
    for (int q = 0; q < kLutPerLane; ++q) {  // (clamped, not predicated: keeps lv[] in registers)
      const int t = (int)threadIdx.x + q * kBlock;
      lv[q] = lsrc[kLutVecs % kBlock == 0 || t < kLutVecs ? t : kLutVecs - 1];
    }
    constexpr int kTabWords = (int)(sizeof(SetTable) / 4), kTabPerLane = (kTabWords + kBlock - 1) / kBlock;
    const uint32_t* tsrc = reinterpret_cast<const uint32_t*>(&p.tab);
    uint32_t tw[kTabPerLane];
#pragma unroll
    for (int q = 0; q < kTabPerLane; ++q)
      tw[q] = (int)threadIdx.x + q * kBlock < kTabWords ? tsrc[threadIdx.x + q * kBlock] : 0u;
#pragma unroll
    for (int q = 0; q < kLutPerLane; ++q)
      if (!(TET_ABLATE & 128) && (kLutVecs % kBlock == 0 || (int)threadIdx.x + q * kBlock < kLutVecs))
        reinterpret_cast<uint4*>(hole_lut)[kLutVec0 + threadIdx.x + q * kBlock] = lv[q];
#pragma unroll
    for (int q = 0; q < kTabPerLane; ++q)
      if ((int)threadIdx.x + q * kBlock < kTabWords) reinterpret_cast<uint32_t*>(&tab)[threadIdx.x + q * kBlock] = tw[q];
    __syncthreads();
  }
  TET_STAMP(1);
  StepCfg cfg = p.cfg;
  if (p.step_counter) {  // wave-uniform: scalar registers
    const uint64_t c = *p.step_counter;
    // (the builtin returns int: without the cast a low half of 2^31 or more sign-extends over the high half)
    const uint64_t idx = (((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(c >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)c)) + p.step_rel;
    cfg.key_step = tet::hash_key(p.seed, idx * 4u + 0u);  // (== tet::step_keys, written out: tetris_entry.hpp)
    cfg.key_policy = tet::hash_key(p.seed, idx * 4u + 3u);
  }
  bool invalid = false, done = false, done_flag = false;
  int lines = 0;
  if (live) {
    tet::StepOut out;
    tet::env_step<W, C, NCH, CR, false, tet::scratch_padded<W, C, NCH, CR>()>(in.col, in.meta, in.exhausted ? -1 : in.action, p.action == nullptr && !in.exhausted,
                             tab, hole_lut, &lane_cols[0][threadIdx.x], kBlock, cfg, p.env_offset + i, in.draw,
                             in.draw_reset, out);
    invalid = out.invalid != 0;
    TET_STAMP(2);
    if (p.obs) {
      float4* o4 = reinterpret_cast<float4*>(p.obs);
      st_off(o4, i * 32u, make_float4(out.obs[0], out.obs[1], out.obs[2], out.obs[3]));
      st_off(o4, i * 32u + 16u, make_float4(out.obs[4], out.obs[5], out.obs[6], out.obs[7]));
    }
    if (!invalid) {
      store_planes<W, C, PACK>(p, i, in.col);
      st_off(p.meta, i * 8u, in.meta);
      done = out.done != 0;
      lines = out.lines;
      if (p.stream) p.cursor[i] = in.cursor + 1 + ((out.done && cfg.auto_reset) ? 1 : 0);  // (== tet::stream_advance)
    }
    done_flag = out.done != 0;  // what the done array holds (an env that was already over reports done again)
    st_off(p.reward, i * 4u, (int32_t)out.reward);
    st_off(p.done, i, (uint8_t)out.done);
    st_off(p.lines, i, (uint8_t)out.lines);
    st_off(p.n_valid, i, (uint8_t)out.n_valid);
    if (p.piece_next) st_off(p.piece_next, i, (uint8_t)out.piece);
    if (p.action_out) st_off(p.action_out, i * 4u, (int32_t)out.action);
  }
  if (!(TET_ABLATE & 8192) && (p.status || p.done_bits)) {
    const unsigned long long done_mask = __ballot(done_flag);  // == tetris_hip_pack_done_bits(done)
    const unsigned n_inv = wave_count(invalid);
    const unsigned n_done = wave_count(done);
    const unsigned n_lines = wave_sum(3, lines);
    const unsigned n_steps = wave_count(live && !invalid);
    if ((threadIdx.x & 63) == 0) {
      uint4 v = in.status;
      v.x += n_inv;
      v.y += n_done;
      v.z += n_lines;
      v.w += n_steps;
      if (p.status) st_off(reinterpret_cast<uint4*>(p.status), (i >> 6) * 16u, v);
      if (p.status_snapshot) st_off(reinterpret_cast<uint4*>(p.status_snapshot), (i >> 6) * 16u, v);
      // done_bits is uint64[ceil(B / 64)]: a wave of the grid that lies wholly past B has no word there (the
      // counter buffers are rounded up to the largest tile, tetris_hip_status_words, and take its zero slot)
      if (p.done_bits && (i & ~63u) < p.B) st_off(p.done_bits, (i >> 6) * 8u, done_mask);
    }
  }
#if TET_STAMPS
  __syncthreads();
  if (threadIdx.x == 0 && blockIdx.x < kStampWgs) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have left the CU
    g_stamps[blockIdx.x * kStampWords + 3] = __builtin_amdgcn_s_memrealtime();
    g_stamps[blockIdx.x * kStampWords + 4] = __builtin_amdgcn_s_getreg(63492);  // HW_REG_HW_ID
    g_stamps[blockIdx.x * kStampWords + 5] = __builtin_amdgcn_s_getreg(63508);  // HW_REG_XCC_ID
  }
#endif
}

// Minimum waves per SIMD the kernels built on tet::afterstates_env are compiled for (= their VGPR budget),
// measured per kernel at 1 Mi envs (profiles/r03_experiments/afterstates_family_waves_sweep.txt).  32-bit
// boards: the afterstate matrix kernel is bound by its row stores and runs best unconstrained (2: ~200
// VGPRs, no spills: 0.43 ms against 0.49 / 0.73 at 3 / 4); the greedy policy kernel at 3 (0.255 ms against
// 0.31 / 0.29 at 2 / 4); the kernels that also step (K greedy steps per launch, rollouts) at 4 (128 VGPRs, a
// few spilled dwords: 0.27 ms per step against 0.33 / 0.29, 9.5 ms against 12.8 / 10.6).  64-bit boards
// (10x40): 2 everywhere -- at 3 the 168-VGPR budget spills 600-870 bytes and every kernel is 1.3-2 x slower.
#ifndef TET_AFTER_WAVES
#define TET_AFTER_WAVES 2
#endif
#ifndef TET_GREEDY_WAVES
#define TET_GREEDY_WAVES 3
#endif
#ifndef TET_STEP_GREEDY_WAVES
#define TET_STEP_GREEDY_WAVES 4
#endif
#ifndef TET_AFTER_WAVES64
#define TET_AFTER_WAVES64 2
#endif
// play_linear_kernel: 0 keeps a lane's eight weights in registers across the step loop, 1 reloads the row in
// every step (an L2 hit).  DESIGN.md section 3.5 has the register and scratch report of both forms.
#ifndef TET_PLAY_RELOAD_W
#define TET_PLAY_RELOAD_W 0
#endif
// A hardware hazard met on the way (round 3): on gfx950 a 64-bit shift -- v_lshlrev_b64, v_lshrrev_b64,
// v_ashrrev_i64 -- whose 32-bit shift amount sits in the LAST vector register of the wave's allocation (v255
// of 256, v167 of 168, v127 of 128) shifts by (v0 & 63) instead whenever another wave shares the SIMD
// (tools/ubench/shift64_last_vgpr.hip: 0 wrong results at one workgroup per compute unit, 4-5 % at eight;
// v_lshlrev_b32, v_mad_u64_u32, v_lshl_add_u64 are not affected).  The kernels of this family fill their
// register budgets, all multiples of the allocation granule, so hipcc (ROCm 7.2) did place shift amounts there:
// get_best_policy / get_after_states / rollouts results were wrong only where two workgroups shared a compute
// unit.  Nothing in the source can keep the allocator off that register (amdgpu_num_vgpr has no effect on these
// kernels), so tetris_amd/build.py patches the device ASSEMBLY of every translation unit before it is assembled
// (patch_last_vgpr_shifts), and tools/check_last_vgpr.py -- run by the CPU tests on the built library --
// disassembles it and fails if one kernel still has the pattern.  DESIGN.md section 3.2.
template <typename W, int C>
constexpr int after_waves(int want) {
  return sizeof(W) == 4 ? want : (want > TET_AFTER_WAVES64 ? TET_AFTER_WAVES64 : want);
}

// K consecutive env-steps of every env in ONE launch, for policies that live in the kernel
// (uniform random / greedy linear): the board and meta stay in registers between steps, every
// step's outputs are written to trajectory buffers [K][B]...; bit-identical to K launches of
// step_kernel with step_idx0, step_idx0 + 1, ...  (the per-step keys are re-derived on device).
template <typename W, int C, int NCH, int POLICY, int CR>
__global__ __launch_bounds__(step_block<W>(), (POLICY == 0 ? step_waves<W, CR>() : after_waves<W, C>(TET_STEP_GREEDY_WAVES))) void step_many_kernel(const StepManyParams q) {
  static_assert(POLICY == 0 || CR == 12, "the greedy policy evaluates terminal afterstates too: 12-row chunks");
  constexpr int kBlock = step_block<W>();  // shadows the file-wide tile size inside this kernel
  const StepParams& p = q.one;
  constexpr bool AFTER = POLICY == 1;  // the greedy policy walks the afterstates: tet::AfterLut tables
  __shared__ StepLds<W, C, kBlock, CR, AFTER> lds;
  SetTable& tab = lds.tab;
  uint8_t* const hole_lut = lds.lut;
  auto& lane_cols = lds.lane_cols;
  static_assert(sizeof(lds.lane_cols) / sizeof(lds.lane_cols[0]) >= (tet::scratch_padded<W, C, NCH, CR, AFTER>() ? C + 3 : C), "the unclamped stamp needs its three columns");
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < p.B;
  constexpr bool PACK = NCH != 0 && !TET_NO_PACK;
  StepInputs<W, C> in;
  load_inputs<W, C, PACK>(p, i, in);
  if (AFTER) stage_after_lut(hole_lut);
  else stage_hole_lut<W, C, NCH, CR>(hole_lut);
  stage_table(tab, p.tab);
  unsigned n_inv = 0, n_done = 0, n_lines = 0, n_steps = 0;
  StepCfg cfg = p.cfg;
#pragma unroll 1
  for (int k = 0; k < q.n_steps; ++k) {
    cfg.key_step = tet::hash_key(q.seed, (q.step_idx0 + (uint64_t)k) * 4u + 0u);  // (== tet::step_keys)
    cfg.key_policy = tet::hash_key(q.seed, (q.step_idx0 + (uint64_t)k) * 4u + 3u);
    bool invalid = false, done = false;
    int lines = 0;
    if (live) {
      int action = -1;
      bool use_policy = true;
      if (POLICY == 1) {  // greedy: first non-terminal action of maximal fitness (== tet::GreedyPick)
        float best = 0.f;
        int best_row = -1;
        tet::afterstates_env<W, C, NCH>(in.col, in.meta, tab, hole_lut, cfg.R, [&](bool has, int, int, float (&f)[8], int, int row, bool is_valid) {
          if (!has) return;
          if (is_valid) {
            const float v = tet::fitness_of(f, q.w);
            if (best_row < 0 || v > best || (v == best && row < best_row)) {
              best = v;
              best_row = row;
            }
          }
        });
        action = best_row;
        use_policy = false;
      }
      tet::StepOut out;
      tet::env_step<W, C, NCH, CR, AFTER, tet::scratch_padded<W, C, NCH, CR, AFTER>()>(in.col, in.meta, action, use_policy, tab, hole_lut, &lane_cols[0][threadIdx.x],
                                          kBlock, cfg, p.env_offset + i, -1, -1, out);
      invalid = out.invalid != 0;
      const uint32_t e = (uint32_t)k * p.B + i;  // element index in the [K][B] trajectory buffers
      if (p.obs) {
        float4* o4 = reinterpret_cast<float4*>(p.obs);
        st_off(o4, e * 32u, make_float4(out.obs[0], out.obs[1], out.obs[2], out.obs[3]));
        st_off(o4, e * 32u + 16u, make_float4(out.obs[4], out.obs[5], out.obs[6], out.obs[7]));
      }
      if (!invalid) {
        done = out.done != 0;
        lines = out.lines;
      }
      st_off(p.reward, e * 4u, (int32_t)out.reward);
      st_off(p.done, e, (uint8_t)out.done);
      st_off(p.lines, e, (uint8_t)out.lines);
      st_off(p.n_valid, e, (uint8_t)out.n_valid);
      if (p.piece_next) st_off(p.piece_next, e, (uint8_t)out.piece);
      if (p.action_out) st_off(p.action_out, e * 4u, (int32_t)out.action);
    }
    n_inv += wave_count(invalid);
    n_done += wave_count(done);
    n_lines += wave_sum(3, lines);
    n_steps += wave_count(live && !invalid);
  }
  if (live) {
    store_planes<W, C, PACK>(p, i, in.col);
    st_off(p.meta, i * 8u, in.meta);
  }
  if (p.status && (threadIdx.x & 63) == 0) {
    uint4 v = in.status;
    v.x += n_inv;
    v.y += n_done;
    v.z += n_lines;
    v.w += n_steps;
    st_off(reinterpret_cast<uint4*>(p.status), (i >> 6) * 16u, v);
  }
}

template <typename W, int C, bool PACK>
__global__ __launch_bounds__(kBlock) void reset_kernel(const ResetParams p) {
  __shared__ SetTable tab;
  stage_table(tab, p.tab);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool mine = i < p.B && !(p.reset_mask && !p.reset_mask[i]);
  const int cur = (mine && p.stream) ? p.cursor[i] : 0;
  const bool exhausted = mine && p.stream && tet::stream_reset_exhausted(cur, p.stream_len);
  if (p.status) {
    const unsigned n_bad = (unsigned)__popcll(__ballot(exhausted));
    if ((threadIdx.x & 63) == 0 && n_bad) p.status[(i >> 6) * 4 + TETRIS_STATUS_INVALID] += n_bad;
  }
  if (!mine || exhausted) return;
  tet::reset_env<W, C, PACK>(static_cast<W*>(p.cols), p.meta, p.B, i, tab, p.init_bag, p.n_pieces, p.key, p.env_offset, p.stream,
                             p.cursor, cur, p.piece_out, p.n_valid_out);
}

template <typename W, int C, bool PACK>
__global__ __launch_bounds__(kBlock) void refresh_kernel(const RefreshParams p) {
  __shared__ SetTable tab;
  stage_table(tab, p.tab);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.B) return;
  tet::refresh_env<W, C, PACK>(static_cast<const W*>(p.cols), p.meta, p.n_valid_out, p.B, i, tab, p.R);
}

// game.py:67-80.  One lane per env walks the static slots in reference order;
// the k-th non-terminal placement lands in feats[i][k].


// Feature rows are 32 bytes and the rows of different envs are far apart, so a plain store of one
// row per lane is 64 separate 16-byte write requests per instruction -- the kernel was bound by
// the L2 write-request rate (75 M requests per launch), not by bytes.  Lanes therefore pair up:
// in two steps the even/odd lane of a pair write the two 16-byte halves of ONE row (first the even
// lane's row, then the odd lane's), so every request carries a whole 32-byte row.  The halves
// change lanes through DPP (quad_perm 1,0,3,2: neighbours swap) -- round 1 sent them through LDS,
// whose write -> wave barrier -> read round trip sat on the critical path of a kernel that is bound
// by latency.  All lanes of the wave must call this together (afterstates_env's emit is
// wave-uniform).
__device__ __forceinline__ uint32_t swap_neighbour(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}
__device__ __forceinline__ void store_row_paired(float* base, bool has, uint32_t at4, const float (&f)[8]) {
  const bool odd = threadIdx.x & 1u;
  const uint32_t at_mine = has ? at4 : ~0u;
  const uint32_t at_other = swap_neighbour(at_mine);
  float r[4];  // the partner's half this lane stores: even lanes get the odd row's low half, odd lanes the even row's high half
#pragma unroll
  for (int q = 0; q < 4; ++q)
    r[q] = __uint_as_float(swap_neighbour(__float_as_uint(odd ? f[q] : f[q + 4])));
  const uint32_t d_even = odd ? at_other : at_mine, d_odd = odd ? at_mine : at_other;  // rows of the pair's even / odd lane
  const float4 v_even = odd ? make_float4(r[0], r[1], r[2], r[3]) : make_float4(f[0], f[1], f[2], f[3]);
  const float4 v_odd = odd ? make_float4(f[4], f[5], f[6], f[7]) : make_float4(r[0], r[1], r[2], r[3]);
  float4* out = reinterpret_cast<float4*>(base);
  const uint32_t part = odd ? 1u : 0u;
  if (d_even != ~0u) out[(size_t)d_even + part] = v_even;
  if (d_odd != ~0u) out[(size_t)d_odd + part] = v_odd;
}

template <typename W, int C, int NCH>
__global__ __launch_bounds__(kBlock, (after_waves<W, C>(TET_AFTER_WAVES))) void afterstates_kernel(const AfterParams p) {
  __shared__ SetTable tab;
  __shared__ __attribute__((aligned(16))) uint8_t hole_lut[tet::kAfterLutBytes];
  stage_after_lut(hole_lut);
  stage_table(tab, p.tab);
  const int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i0 < p.B;
  const int64_t i = live ? i0 : p.B - 1;  // lanes past the end keep pace on the last env and store nothing
  const W* cols = static_cast<const W*>(p.cols);
  W col[C];
  tet::load_board<W, C, (NCH != 0 && !TET_NO_PACK)>(cols, p.B, i, col);
  const uint64_t meta = p.meta[i];
  const int piece = tet::meta_piece(meta);
  const uint64_t full = tab.fullmask[piece];
  const uint64_t valid = tet::meta_mask(meta) & full;  // non-terminal slots (kept fresh by step/reset/refresh)
  // env-major ([B][a_max][8]: row_stride 8) keeps a wave's 36 rows x 64 envs inside one 72 KiB
  // span; action-major ([a_max][B][8]: env_stride 8) walks 36 regions 32 MiB apart and measured
  // 1.4x slower (TLB reach), so env-major is the default upstream.  Offsets are in float4 units
  // (the C-ABI checks that the whole matrix stays below 2^32 of them).
  const uint32_t es4 = (uint32_t)(p.env_stride / 4), rs4 = (uint32_t)(p.row_stride / 4);
  const uint32_t env4 = (uint32_t)i * es4;
  const int nv = tet::popc(valid), na = tet::popc(full);
  float sink = 0.f;
  tet::afterstates_env<W, C, NCH>(col, meta, tab, hole_lut, p.R, [&](bool has, int sk, int sc, float (&f)[8], int row_all, int row_valid, bool is_valid) {
    has = has && live;
    if (TET_ABLATE & 64) {  // timing experiment: no feature stores
      if (has) sink += f[0] + f[1] + f[2] + f[3] + f[4] + f[5] + f[6] + f[7] + (float)(sk + sc);
      return;
    }
    if (p.has_direct_by) {
#pragma unroll
      for (int q = 0; q < 8; ++q) f[q] *= p.direct_by[q];
    }
    // the row of a placement follows the reference's enumeration order
    if (p.feats_all) store_row_paired(p.feats_all, has, env4 + (uint32_t)row_all * rs4, f);
    store_row_paired(p.feats, has && is_valid, env4 + (uint32_t)row_valid * rs4, f);  // game.py:69
  });
  if (TET_ABLATE & 64) {
    if (live) p.feats[i * p.env_stride] = sink;
    return;
  }
  // zero the rows past the last placement: the lanes of a pair write the two halves of one row per
  // instruction as above, but there is nothing to exchange -- only the partner's base, count and liveness,
  // fetched once
  {
    const bool odd = threadIdx.x & 1u;
    const uint32_t part = odd ? 1u : 0u;
    const uint32_t env4_o = swap_neighbour(env4);
    const int nv_o = (int)swap_neighbour((uint32_t)(live ? nv : 0x7FFFFFFF)), na_o = (int)swap_neighbour((uint32_t)(live ? na : 0x7FFFFFFF));
    const int nv_m = live ? nv : 0x7FFFFFFF, na_m = live ? na : 0x7FFFFFFF;
    // rows of the pair's even / odd lane
    const uint32_t base_e = odd ? env4_o : env4, base_o = odd ? env4 : env4_o;
    const int nv_e = odd ? nv_o : nv_m, nv_od = odd ? nv_m : nv_o, na_e = odd ? na_o : na_m, na_od = odd ? na_m : na_o;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4* out = reinterpret_cast<float4*>(p.feats);
    float4* out_all = reinterpret_cast<float4*>(p.feats_all);
    for (int k = 0; k < p.a_max; ++k) {  // (wave-uniform loop)
      const uint32_t r4 = (uint32_t)k * rs4 + part;
      if (k >= nv_e) out[(size_t)base_e + r4] = z4;
      if (k >= nv_od) out[(size_t)base_o + r4] = z4;
      if (out_all) {
        if (k >= na_e) out_all[(size_t)base_e + r4] = z4;
        if (k >= na_od) out_all[(size_t)base_o + r4] = z4;
      }
    }
  }
  if (live) {
    p.n_valid[i] = (uint8_t)nv;
    if (p.n_all) p.n_all[i] = (uint8_t)na;
  }
}


// Tetris.get_best_policy / fitness (game.py:102-120) for every env: the fitness of every
// placement (raw order, terminal included, like game.py:103) and the best NON-terminal action.
// The [B][a_max][8] feature matrix never touches HBM.
template <typename W, int C, int NCH>
__global__ __launch_bounds__(kBlock, (after_waves<W, C>(TET_GREEDY_WAVES))) void greedy_kernel(const GreedyParams p) {
  __shared__ SetTable tab;
  __shared__ __attribute__((aligned(16))) uint8_t hole_lut[tet::kAfterLutBytes];
  stage_after_lut(hole_lut);
  stage_table(tab, p.tab);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.B) return;
  const W* cols = static_cast<const W*>(p.cols);
  W col[C];
  tet::load_board<W, C, (NCH != 0 && !TET_NO_PACK)>(cols, p.B, i, col);
  const uint64_t meta = p.meta[i];
  const int piece = tet::meta_piece(meta);
  const uint64_t full = tab.fullmask[piece];
  const uint64_t valid = tet::meta_mask(meta) & full;
  float* fall = p.fitness_all ? p.fitness_all + i * (int64_t)p.a_max : nullptr;
  tet::GreedyPick pick;
  tet::afterstates_env<W, C, NCH>(col, meta, tab, hole_lut, p.R, [&](bool has, int, int, float (&f)[8], int row_all, int row, bool is_valid) {
    if (!has) return;
    const float v = tet::fitness_of(f, p.w);
    if (fall && !(TET_ABLATE & 2048)) fall[row_all] = v;
    if (is_valid) pick.offer(v, row);
  });
  if (fall)
    for (int k = tet::popc(full); k < p.a_max; ++k) fall[k] = 0.f;
  p.best_action[i] = pick.best_row;
  if (p.best_value) p.best_value[i] = pick.best;
}

// greedy_kernel with the weight row taken per env from a device matrix (tet::load_weight_row: two 16-byte loads
// per lane, issued with the board's).  An env whose row is outside [0, P) writes nothing and goes to its wave's
// counter slot like gather_envs_kernel's bad entries.  No lane leaves early: the ballot sees the whole wave.
template <typename W, int C, int NCH>
__global__ __launch_bounds__(kBlock, (after_waves<W, C>(TET_GREEDY_WAVES))) void greedy_rows_kernel(const GreedyRowsParams p) {
  __shared__ SetTable tab;
  __shared__ __attribute__((aligned(16))) uint8_t hole_lut[tet::kAfterLutBytes];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < p.B;
  const int32_t row = !live ? -1 : (p.rows ? p.rows[i] : (int32_t)i);
  const bool ok = live && tet::weight_row_ok(row, p.P);
  float w[8];
  tet::load_weight_row(p.weights, ok ? row : 0, w);
  stage_after_lut(hole_lut);
  stage_table(tab, p.tab);
  if (ok) {
    W col[C];
    tet::load_board<W, C, (NCH != 0 && !TET_NO_PACK)>(static_cast<const W*>(p.cols), p.B, i, col);
    const tet::GreedyPick pick = tet::greedy_pick_env<W, C, NCH>(col, p.meta[i], tab, hole_lut, p.R, w);
    p.best_action[i] = pick.best_row;
    if (p.best_value) p.best_value[i] = pick.best;
  }
  if (p.status) {
    const unsigned n_bad = wave_count(live && !ok);
    if ((threadIdx.x & 63) == 0 && n_bad) p.status[(i >> 6) * 4 + TETRIS_STATUS_INVALID] += n_bad;
  }
}

// n_steps greedy steps of every env on ITS weight row in one launch (tetris_hip_play_linear): step_many_kernel's
// greedy variant without the trajectory -- board and meta in registers between the steps, per-env totals at the
// end -- and without auto-reset: a lane whose env is over skips the body for the rest of the launch.  The trip
// count is n_steps whatever the games do; the wave counters stay outside the divergent body.  The eight weights
// are loaded once in front of the loop and stay in registers (DESIGN.md section 3.5 has the register report).
template <typename W, int C, int NCH>
__global__ __launch_bounds__(step_block<W>(), (after_waves<W, C>(TET_STEP_GREEDY_WAVES))) void play_linear_kernel(const PlayParams p) {
  constexpr int kBlock = step_block<W>();  // shadows the file-wide tile size inside this kernel
  __shared__ StepLds<W, C, kBlock, 12, true> lds;
  SetTable& tab = lds.tab;
  uint8_t* const hole_lut = lds.lut;
  auto& lane_cols = lds.lane_cols;
  constexpr bool SPAD = tet::scratch_padded<W, C, NCH, 12, true>();
  static_assert(sizeof(lds.lane_cols) / sizeof(lds.lane_cols[0]) >= (SPAD ? C + 3 : C), "the unclamped stamp needs its three columns");
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < p.B;
  const uint32_t ii = live ? i : 0;
  const bool wave_live = (i & ~63u) < p.B;  // (wave-uniform) this wave holds envs: it has a counter slot to keep
  constexpr bool PACK = NCH != 0 && !TET_NO_PACK;
  constexpr int NP = tet::n_planes(C, PACK);
  // every global load of the lane first: board, meta, its row index and weights, the wave's counters
  const uint32_t rec = record_off<W, NP>(ii);
  W col[C];
  {
    W pl[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) pl[q] = ld_off(static_cast<const W*>(p.cols), rec + (uint32_t)(q * 64 * sizeof(W)));
    tet::unpack_board<W, C, PACK>(pl, col);
  }
  uint64_t meta = ld_off(p.meta, ii * 8u);
  const int32_t row = p.rows ? ld_off(p.rows, ii * 4u) : (int32_t)ii;
  const bool ok = live && tet::weight_row_ok(row, p.P);
  float w[8];
  if (!TET_PLAY_RELOAD_W) tet::load_weight_row(p.weights, ok ? row : 0, w);
  uint4 slot = make_uint4(0, 0, 0, 0);
  if (p.status && wave_live) slot = ld_off(reinterpret_cast<const uint4*>(p.status), (i >> 6) * 16u);
  stage_after_lut(hole_lut);
  stage_table(tab, p.tab);
  unsigned n_done = 0, n_lines = 0, n_steps = 0;
  uint32_t my_lines = 0, my_pieces = 0;
  tet::StepCfg cfg = p.cfg;
#pragma unroll 1
  for (int k = 0; k < p.n_steps; ++k) {
    cfg.key_step = tet::hash_key(p.seed, (p.step_idx0 + (uint64_t)k) * 4u + 0u);  // (== tet::step_keys)
    cfg.key_policy = tet::hash_key(p.seed, (p.step_idx0 + (uint64_t)k) * 4u + 3u);
    bool stepped = false, done = false;
    int lines = 0;
    if (ok && !tet::env_over(meta)) {
      if (TET_PLAY_RELOAD_W) tet::load_weight_row(p.weights, row, w);
      tet::StepOut out;
      tet::play_step_env<W, C, NCH, SPAD>(col, meta, w, tab, hole_lut, &lane_cols[0][threadIdx.x], kBlock, cfg,
                                          p.env_offset + i, out);
      if (!out.invalid) {
        stepped = true;
        done = out.done != 0;
        lines = out.lines;
        my_lines += (uint32_t)out.lines;
        my_pieces += 1;
      }
    }
    n_done += wave_count(done);
    n_lines += wave_sum(3, lines);
    n_steps += wave_count(stepped);
  }
  if (my_pieces) {  // an env that was over at entry keeps every byte
    W pl[NP];
    tet::pack_board<W, C, PACK>(col, pl);
#pragma unroll
    for (int q = 0; q < NP; ++q) st_off(static_cast<W*>(p.cols), rec + (uint32_t)(q * 64 * sizeof(W)), pl[q]);
    st_off(p.meta, i * 8u, meta);
    st_off(p.lines_total, i * 4u, ld_off(p.lines_total, i * 4u) + my_lines);
    st_off(p.pieces_total, i * 4u, ld_off(p.pieces_total, i * 4u) + my_pieces);
  }
  if (ok) {
    if (p.n_valid) st_off(p.n_valid, i, (uint8_t)tet::popc(tet::meta_mask(meta)));
    if (p.piece) st_off(p.piece, i, (uint8_t)tet::meta_piece(meta));
  }
  const unsigned n_inv = wave_count(live && !ok);
  if (p.status && wave_live && (threadIdx.x & 63) == 0) {
    slot.x += n_inv;
    slot.y += n_done;
    slot.z += n_lines;
    slot.w += n_steps;
    st_off(reinterpret_cast<uint4*>(p.status), (i >> 6) * 16u, slot);
  }
}

// One sampled decision per env from the softmax of its weight row's logits (tetris_hip_policy_softmax_rows):
// greedy_rows_kernel with tet::softmax_pick_env as the reduction -- the same launch bounds, the same LDS (tables
// only, nothing per lane), the same contract for a row outside [0, P).  The feature matrix never reaches memory;
// an env writes 4 + 4 (+ 32 + 4) bytes, and its row of logits only when asked.
template <typename W, int C, int NCH>
__global__ __launch_bounds__(kBlock, (after_waves<W, C>(TET_GREEDY_WAVES))) void softmax_rows_kernel(const SoftmaxRowsParams p) {
  __shared__ SetTable tab;
  __shared__ __attribute__((aligned(16))) uint8_t hole_lut[tet::kAfterLutBytes];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < p.B;
  const int32_t row = !live ? -1 : (p.rows ? p.rows[i] : (int32_t)i);
  const bool ok = live && tet::weight_row_ok(row, p.P);
  float w[8];
  tet::load_weight_row(p.weights, ok ? row : 0, w);
  stage_after_lut(hole_lut);
  stage_table(tab, p.tab);
  if (ok) {
    W col[C];
    tet::load_board<W, C, (NCH != 0 && !TET_NO_PACK)>(static_cast<const W*>(p.cols), p.B, i, col);
    const uint64_t meta = p.meta[i];
    float* lrow = p.logits ? p.logits + i * (int64_t)p.a_max : nullptr;
    tet::SoftmaxPick pick;
    tet::softmax_pick_env<W, C, NCH>(col, meta, tab, hole_lut, p.R, w, p.inv_t, p.has_direct_by != 0, p.direct_by, p.key,
                                     p.env_offset + (uint32_t)i, lrow, pick);
    if (lrow) {
      const float ninf = -__builtin_inff();
      for (int k = tet::popc(tet::meta_mask(meta) & tab.fullmask[tet::meta_piece(meta)]); k < p.a_max; ++k) lrow[k] = ninf;
    }
    p.action[i] = pick.action;
    p.logp[i] = pick.logp;
    if (p.logz) p.logz[i] = pick.logz;
    if (p.score) {
      float4* dst = reinterpret_cast<float4*>(p.score) + 2 * i;
      dst[0] = make_float4(pick.score[0], pick.score[1], pick.score[2], pick.score[3]);
      dst[1] = make_float4(pick.score[4], pick.score[5], pick.score[6], pick.score[7]);
    }
  }
  if (p.status) {
    const unsigned n_bad = wave_count(live && !ok);
    if ((threadIdx.x & 63) == 0 && n_bad) p.status[(i >> 6) * 4 + TETRIS_STATUS_INVALID] += n_bad;
  }
}

// n_steps SAMPLED steps of every env on its weight row in one launch (tetris_hip_play_softmax): play_linear_kernel
// with the pick replaced by tet::softmax_pick_env.  The running sums of logp and of the score start from the
// totals in memory and take one float32 addition per placed piece, in step order, so launches compose bit for bit.
template <typename W, int C, int NCH>
__global__ __launch_bounds__(step_block<W>(), (after_waves<W, C>(TET_STEP_GREEDY_WAVES))) void play_softmax_kernel(const PlaySoftmaxParams q) {
  const PlayParams& p = q.play;
  constexpr int kBlock = step_block<W>();  // shadows the file-wide tile size inside this kernel
  __shared__ StepLds<W, C, kBlock, 12, true> lds;
  SetTable& tab = lds.tab;
  uint8_t* const hole_lut = lds.lut;
  auto& lane_cols = lds.lane_cols;
  constexpr bool SPAD = tet::scratch_padded<W, C, NCH, 12, true>();
  static_assert(sizeof(lds.lane_cols) / sizeof(lds.lane_cols[0]) >= (SPAD ? C + 3 : C), "the unclamped stamp needs its three columns");
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < p.B;
  const uint32_t ii = live ? i : 0;
  const bool wave_live = (i & ~63u) < p.B;  // (wave-uniform) this wave holds envs: it has a counter slot to keep
  constexpr bool PACK = NCH != 0 && !TET_NO_PACK;
  constexpr int NP = tet::n_planes(C, PACK);
  const uint32_t rec = record_off<W, NP>(ii);
  W col[C];
  {
    W pl[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) pl[k] = ld_off(static_cast<const W*>(p.cols), rec + (uint32_t)(k * 64 * sizeof(W)));
    tet::unpack_board<W, C, PACK>(pl, col);
  }
  uint64_t meta = ld_off(p.meta, ii * 8u);
  const int32_t row = p.rows ? ld_off(p.rows, ii * 4u) : (int32_t)ii;
  const bool ok = live && tet::weight_row_ok(row, p.P);
  float w[8];
  tet::load_weight_row(p.weights, ok ? row : 0, w);
  float my_logp = q.logp_total ? ld_off(q.logp_total, ii * 4u) : 0.f;
  float my_score[8];
  {
    const float4 lo = ld_off(reinterpret_cast<const float4*>(q.score_total), ii * 32u);
    const float4 hi = ld_off(reinterpret_cast<const float4*>(q.score_total), ii * 32u + 16u);
    my_score[0] = lo.x, my_score[1] = lo.y, my_score[2] = lo.z, my_score[3] = lo.w;
    my_score[4] = hi.x, my_score[5] = hi.y, my_score[6] = hi.z, my_score[7] = hi.w;
  }
  uint4 slot = make_uint4(0, 0, 0, 0);
  if (p.status && wave_live) slot = ld_off(reinterpret_cast<const uint4*>(p.status), (i >> 6) * 16u);
  stage_after_lut(hole_lut);
  stage_table(tab, p.tab);
  unsigned n_done = 0, n_lines = 0, n_steps = 0;
  uint32_t my_lines = 0, my_pieces = 0;
  tet::StepCfg cfg = p.cfg;
#pragma unroll 1
  for (int k = 0; k < p.n_steps; ++k) {
    cfg.key_step = tet::hash_key(p.seed, (p.step_idx0 + (uint64_t)k) * 4u + 0u);  // (== tet::step_keys)
    cfg.key_policy = tet::hash_key(p.seed, (p.step_idx0 + (uint64_t)k) * 4u + 3u);
    const uint32_t key_sample = tet::softmax_key(p.seed, p.step_idx0 + (uint64_t)k);
    bool stepped = false, done = false;
    int lines = 0;
    if (ok && !tet::env_over(meta)) {
      tet::SoftmaxPick pick;
      tet::StepOut out;
      tet::play_softmax_step_env<W, C, NCH, SPAD>(col, meta, w, q.inv_t, key_sample, tab, hole_lut, &lane_cols[0][threadIdx.x],
                                                  kBlock, cfg, p.env_offset + i, pick, out);
      if (!out.invalid) {
        stepped = true;
        done = out.done != 0;
        lines = out.lines;
        my_lines += (uint32_t)out.lines;
        my_pieces += 1;
        my_logp = TET_FADD(my_logp, pick.logp);
#pragma unroll
        for (int j = 0; j < 8; ++j) my_score[j] = TET_FADD(my_score[j], pick.score[j]);
      }
    }
    n_done += wave_count(done);
    n_lines += wave_sum(3, lines);
    n_steps += wave_count(stepped);
  }
  if (my_pieces) {  // an env that was over at entry keeps every byte
    W pl[NP];
    tet::pack_board<W, C, PACK>(col, pl);
#pragma unroll
    for (int k = 0; k < NP; ++k) st_off(static_cast<W*>(p.cols), rec + (uint32_t)(k * 64 * sizeof(W)), pl[k]);
    st_off(p.meta, i * 8u, meta);
    st_off(p.lines_total, i * 4u, ld_off(p.lines_total, i * 4u) + my_lines);
    st_off(p.pieces_total, i * 4u, ld_off(p.pieces_total, i * 4u) + my_pieces);
    if (q.logp_total) st_off(q.logp_total, i * 4u, my_logp);
    st_off(reinterpret_cast<float4*>(q.score_total), i * 32u, make_float4(my_score[0], my_score[1], my_score[2], my_score[3]));
    st_off(reinterpret_cast<float4*>(q.score_total), i * 32u + 16u, make_float4(my_score[4], my_score[5], my_score[6], my_score[7]));
  }
  if (ok) {
    if (p.n_valid) st_off(p.n_valid, i, (uint8_t)tet::popc(tet::meta_mask(meta)));
    if (p.piece) st_off(p.piece, i, (uint8_t)tet::meta_piece(meta));
  }
  const unsigned n_inv = wave_count(live && !ok);
  if (p.status && wave_live && (threadIdx.x & 63) == 0) {
    slot.x += n_inv;
    slot.y += n_done;
    slot.z += n_lines;
    slot.w += n_steps;
    st_off(reinterpret_cast<uint4*>(p.status), (i >> 6) * 16u, slot);
  }
}

// Tetris.perform_rollouts (game.py:150-160) as a fan-out: one lane per (env, first action) runs its
// n rollouts back to back with the board in registers; nothing but the mean returns is written.
// 512 lanes per workgroup: with the 35 KiB of afterstate tables two workgroups = 16 waves fit a CU
constexpr int kRolloutBlock = 512;
template <typename W, int C, int NCH>
__global__ __launch_bounds__(kRolloutBlock, (after_waves<W, C>(TET_STEP_GREEDY_WAVES))) void rollouts_kernel(const RolloutParams p) {
  constexpr int kBlock = kRolloutBlock;  // shadows the file-wide tile size inside this kernel
  __shared__ StepLds<W, C, kBlock, 12, true> lds;
  SetTable& tab = lds.tab;
  uint8_t* const hole_lut = lds.lut;
  auto& lane_cols = lds.lane_cols;
  stage_after_lut(hole_lut);
  stage_table(tab, p.tab);
  const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (id >= p.B * p.a_max) return;
  const int64_t i = id / p.a_max;
  const int a0 = (int)(id - i * p.a_max);
  const W* cols = static_cast<const W*>(p.cols);
  W col[C];
  tet::load_board<W, C, (NCH != 0 && !TET_NO_PACK)>(cols, p.B, i, col);
  const uint64_t meta = p.meta[i];
  // (== tet::rollout_mean, written out: tetris_entry.hpp)
  const int nv = tet::popc(tet::meta_mask(meta));
  double mean = __longlong_as_double(0x7FF8000000000000ll);  // NaN: not an action of this env
  if (a0 < nv) {
    int sum = 0;
    for (int r = 0; r < p.n; ++r) {
      const uint64_t uid = ((uint64_t)(p.env_offset + i) * (uint64_t)p.a_max + (uint64_t)a0) * (uint64_t)p.n + r;
      const uint32_t key0 = tet::mix32(p.key ^ ((uint32_t)(uid >> 32) * 0x9E3779B1u));
      const uint64_t fed = ((uint64_t)(i * p.a_max + a0) * (uint64_t)p.n + (uint64_t)r) * (uint64_t)p.length;
      sum += tet::rollout_env<W, C, NCH>(col, meta, a0, p.length, p.policy, p.w, tab, hole_lut,
                                    &lane_cols[0][threadIdx.x], kBlock, p.R, p.n_pieces, key0, (uint32_t)uid,
                                    p.pieces ? p.pieces + fed : nullptr);
    }
    mean = (double)sum / (double)p.n;
  }
  p.returns[id] = mean;
}

// Two-piece lookahead of every env in one launch (tetris_hip_policy_two_ply): rollouts_kernel's fan-out -- one lane per
// (env, first action), its tile, its LDS block, the afterstate tables -- with whole envs per workgroup: EPB =
// kRolloutBlock / a_max envs, lane e * a_max + k being action k of the workgroup's e-th env; the lanes behind the last
// whole env (a_max - 1 at the most) idle.  A lane stamps its placement once and evaluates every piece of the set on the
// child in registers (tet::two_ply_lane); the child never reaches memory.  The sums of a workgroup meet in LDS, and
// after one barrier the first EPB lanes each pick for one env (tet::two_ply_pick).  No lane leaves early: the staging,
// both barriers and the pick sit outside every branch.  Plain stores only, none for a lane or an env past B.
template <typename W, int C, int NCH>
__global__ __launch_bounds__(kRolloutBlock, (after_waves<W, C>(TET_STEP_GREEDY_WAVES))) void two_ply_kernel(const TwoPlyParams p) {
  constexpr int kBlock = kRolloutBlock;  // shadows the file-wide tile size inside this kernel
  __shared__ StepLds<W, C, kBlock, 12, true> lds;
  __shared__ float q_lds[kBlock];
  SetTable& tab = lds.tab;
  uint8_t* const hole_lut = lds.lut;
  auto& lane_cols = lds.lane_cols;
  constexpr bool SPAD = tet::scratch_padded<W, C, NCH, 12, true>();
  static_assert(sizeof(lds.lane_cols) / sizeof(lds.lane_cols[0]) >= (SPAD ? C + 3 : C), "the unclamped stamp needs its three columns");
  const int epb = kBlock / p.a_max;
  const int e = (int)threadIdx.x / p.a_max;
  const int k = (int)threadIdx.x - e * p.a_max;
  const int64_t i = (int64_t)blockIdx.x * epb + e;
  const bool live = e < epb && i < p.B;
  const int64_t ii = live ? i : 0;  // (an env every launch has: the loads sit in front of the staging)
  W col[C];
  tet::load_board<W, C, (NCH != 0 && !TET_NO_PACK)>(static_cast<const W*>(p.cols), p.B, ii, col);
  const uint64_t meta = p.meta[ii];
  stage_after_lut(hole_lut);
  stage_table(tab, p.tab);
  float q = __builtin_nanf("");
  if (live) {
    const int64_t at = i * p.a_max + k;
    q = tet::two_ply_lane<W, C, NCH, SPAD>(col, meta, k, tet::two_ply_bag(meta, p.n_pieces), p.w, p.death_value, p.n_pieces, tab,
                                           hole_lut, &lane_cols[0][threadIdx.x], kBlock, p.R,
                                           p.values ? p.values + at * p.n_pieces : nullptr);
    if (p.q) p.q[at] = q;
  }
  q_lds[threadIdx.x] = q;
  __syncthreads();
  const int64_t i2 = (int64_t)blockIdx.x * epb + threadIdx.x;
  if ((int)threadIdx.x < epb && i2 < p.B) {
    const uint64_t m2 = p.meta[i2];
    const tet::GreedyPick pick = tet::two_ply_pick(&q_lds[threadIdx.x * p.a_max], tet::two_ply_n_valid(m2, p.a_max));
    if (p.n_bag) p.n_bag[i2] = (uint8_t)tet::popc(tet::two_ply_bag(m2, p.n_pieces));
    if (p.best_action) p.best_action[i2] = pick.best_row;
    if (p.best_value) p.best_value[i2] = pick.best;
  }
}

// dst env j := src env index[j] (tet::gather_env), one lane per dst env, for any column count: the planes are
// opaque words, NP of them (tet::gather_variant).  The index load (coalesced) is in flight while the twelve fullmask words are staged; the body then
// issues the gathered plane and meta loads back to back and stores the dst tile record, meta, n_valid and piece
// coalesced.  Padding lanes take the "keep" path, so nothing past B_dst is written.  Invalid entries go to the
// wave's own counter slot like the step's: ballot, popcount, a plain read-modify-write by lane 0.
template <typename W, int NP>
__global__ __launch_bounds__(kBlock) void gather_envs_kernel(const GatherParams p) {
  __shared__ uint64_t fullmask[tet::kMetaPieces];
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int32_t idx = j < p.B_dst ? p.index[j] : -1;
  if (threadIdx.x < tet::kMetaPieces) fullmask[threadIdx.x] = p.fullmask[threadIdx.x];
  __syncthreads();
  const bool invalid = tet::gather_env<W, NP>(static_cast<const W*>(p.src_cols), p.src_meta, p.B_src, static_cast<W*>(p.dst_cols),
                                              p.dst_meta, p.dst_n_valid, p.dst_piece, idx, j, fullmask);
  if (p.status) {
    const unsigned n_bad = wave_count(invalid);
    if ((threadIdx.x & 63) == 0 && n_bad) p.status[(j >> 6) * 4 + TETRIS_STATUS_INVALID] += n_bad;
  }
}

// dst env j := src env parent[j] after placement action[j] (tetris_hip_expand_envs): gather_envs_kernel's scattered
// read joined to step_kernel's body, on step_kernel's instantiation, feature tables and 256-env tile, so the board of
// a child goes from the parent's registers to dst without a copy in HBM in between.  One lane per dst env.  The lane's
// three index loads are coalesced; the gathered plane loads (a compile-time count) and the gathered meta load follow
// back to back, clamped to src env 0 for the lanes that run nothing, so that the staging and its barrier sit outside
// every branch.  Kept and bad entries and the lanes past B_dst store nothing; bad entries go to the wave's counter slot
// like gather_envs_kernel's.
template <typename W, int C, int NCH, int CR, bool PACK>
__global__ __launch_bounds__(kBlock, (step_waves<W, CR>())) void expand_kernel(const ExpandParams p) {
  __shared__ StepLds<W, C, kBlock, CR> lds;
  SetTable& tab = lds.tab;
  uint8_t* const hole_lut = lds.lut;
  auto& lane_cols = lds.lane_cols;
  constexpr bool SPAD = tet::scratch_padded<W, C, NCH, CR>();
  static_assert(sizeof(lds.lane_cols) / sizeof(lds.lane_cols[0]) >= (SPAD ? C + 3 : C), "the unclamped stamp needs its three columns");
  static_assert(PACK == (NCH != 0 && !TET_NO_PACK), "a counted-chunk variant runs exactly on packed boards");
  constexpr int NP = tet::n_planes(C, PACK);
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  const bool live = j < p.B_dst;
  const uint32_t jj = live ? j : 0;
  const int32_t parent = live ? ld_off(p.parent, jj * 4u) : -1;
  const int action = ld_off(p.action, jj * 4u);
  const int next_piece = p.next_piece ? (int)ld_off(p.next_piece, jj) : -1;
  const int entry = tet::expand_entry(parent, p.B_src, next_piece, p.cfg.n_pieces);
  const bool run = entry == tet::kExpandRun;
  const uint32_t ii = run ? (uint32_t)parent : 0u;  // (a src env every launch has)
  const uint32_t src_rec = record_off<W, NP>(ii);
  W pl[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) pl[q] = ld_off(static_cast<const W*>(p.src_cols), src_rec + (uint32_t)(q * 64 * sizeof(W)));
  uint64_t meta = ld_off(p.src_meta, ii * 8u);
  stage_hole_lut<W, C, NCH, CR>(hole_lut);
  stage_table(tab, p.tab);
  bool bad = entry == tet::kExpandBad;
  if (run) {
    W col[C];
    tet::unpack_board<W, C, PACK>(pl, col);
    tet::StepOut out;
    tet::expand_env<W, C, NCH, CR, SPAD>(col, meta, action, next_piece, tab, hole_lut, &lane_cols[0][threadIdx.x], kBlock, p.cfg,
                                         p.env_offset + ii, out);
    bad = out.invalid != 0;
    if (!bad) {
      tet::pack_board<W, C, PACK>(col, pl);
      const uint32_t dst_rec = record_off<W, NP>(j);
#pragma unroll
      for (int q = 0; q < NP; ++q) st_off(static_cast<W*>(p.dst_cols), dst_rec + (uint32_t)(q * 64 * sizeof(W)), pl[q]);
      st_off(p.dst_meta, j * 8u, meta);
      if (p.obs) {
        float4* o4 = reinterpret_cast<float4*>(p.obs);
        st_off(o4, j * 32u, make_float4(out.obs[0], out.obs[1], out.obs[2], out.obs[3]));
        st_off(o4, j * 32u + 16u, make_float4(out.obs[4], out.obs[5], out.obs[6], out.obs[7]));
      }
      st_off(p.reward, j * 4u, (int32_t)out.reward);
      st_off(p.done, j, (uint8_t)out.done);
      st_off(p.lines, j, (uint8_t)out.lines);
      st_off(p.n_valid, j, (uint8_t)out.n_valid);
      st_off(p.piece, j, (uint8_t)out.piece);
    }
  }
  if (p.status) {
    const unsigned n_bad = wave_count(bad);
    if ((threadIdx.x & 63) == 0 && n_bad) p.status[(j >> 6) * 4 + TETRIS_STATUS_INVALID] += n_bad;
  }
}

__global__ void counter_add_kernel(uint64_t* counter, uint64_t n) { *counter += n; }

// done flags -> bitmask (bit i % 8 of byte i / 8): one ballot per wavefront, eight bytes per store.
// The payload of the done/reset gather, the path's only collective.
__global__ __launch_bounds__(kBlock) void pack_done_bits_kernel(const uint8_t* __restrict__ done,
                                                                unsigned long long* __restrict__ bits, int64_t B) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const unsigned long long m = __ballot(i < B && done[i] != 0);
  if ((threadIdx.x & 63) == 0 && (i & ~(int64_t)63) < B) bits[i >> 6] = m;
}

__global__ __launch_bounds__(kBlock) void policy_random_kernel(const uint8_t* __restrict__ n_valid,
                                                               int32_t* __restrict__ action, uint32_t key,
                                                               int64_t env_offset, int64_t B) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= B) return;
  action[i] = tet::policy_random(key, (uint32_t)(env_offset + i), n_valid[i]);
}

// tet::numpy_bag_stream_env, one lane per env with the generator state in private memory: this is a set-up
// kernel for exact replays of seeded reference games (small to moderate B), not a hot path -- the
// counter-based bag in `meta` is the one for large batches.
__global__ __launch_bounds__(64) void numpy_bag_stream_kernel(const uint32_t* __restrict__ seeds, int n_pieces,
                                                             int64_t L, uint8_t* __restrict__ stream, int64_t B) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i < B) tet::numpy_bag_stream_env(seeds, n_pieces, L, stream, B, i);
}

template <typename W>
__global__ __launch_bounds__(kBlock) void decode_kernel(const W* __restrict__ cols, int8_t* __restrict__ cells,
                                                        int32_t* __restrict__ heights, int C, int rows, int64_t B,
                                                        bool packed) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= B) return;
  for (int c = 0; c < C; ++c) {
    const W x = tet::load_column_rt<W>(cols, B, i, c, C, packed);
    if (heights) heights[i * C + c] = tet::bitlen(x);
    if (cells)
      for (int r = 0; r < rows; ++r) cells[(i * rows + r) * C + c] = (int8_t)((x >> r) & 1);
  }
}

template <typename W>
__global__ __launch_bounds__(kBlock) void encode_kernel(const int8_t* __restrict__ cells, W* __restrict__ cols,
                                                        int C, int rows, int64_t B, bool packed) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= B) return;
  W col[tet::kMaxCols];
  for (int c = 0; c < C; ++c) {
    W x = 0;
    for (int r = 0; r < rows; ++r) x |= (W)(cells[(i * rows + r) * C + c] != 0) << r;
    col[c] = x;
  }
  tet::store_columns_rt<W>(cols, B, i, col, C, packed);
}

// ---- dispatch on (word, C) -------------------------------------------------------

inline dim3 grid_for(int64_t B) { return dim3((unsigned)((B + kBlock - 1) / kBlock)); }
inline dim3 rollout_grid(int64_t n) { return dim3((unsigned)((n + kRolloutBlock - 1) / kRolloutBlock)); }
constexpr uint32_t kSmallBatch = 65536;
template <typename W>
inline dim3 step_grid(int64_t B) { return dim3((unsigned)((B + step_block<W>() - 1) / step_block<W>())); }

// ---- translation units ------------------------------------------------------------------------
// The kernels are templates on the column count, and one hipcc process compiling all of them takes
// minutes, so the in-tree build (tetris_amd/build.py) compiles this file once per column count
// (-DTET_PART=<C>: the kernels of that count behind tetris_part_<C>) plus once as the main unit
// (-DTET_SPLIT_MAIN: the C-ABI -- tetris_abi.inc on the backend at the end of this file -- which reaches the
// column-specific launches through those entries), in parallel, and links the objects.  Compiled alone with neither macro the file is a complete
// single-unit library (what the tools' experiment builds do).
template <template <typename, int> class Launcher> struct LaunchId;
// Which instantiation a geometry runs is tet::kernel_variant's choice (tetris_entry.hpp), for these launchers as
// for the CPU harness; only the tile size of the step kernel is decided here.
template <typename W, int C>
struct LaunchStep {
  static void run(const StepParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.cfg.R, [&](auto nch, auto cr, auto) {
      constexpr int NCH = decltype(nch)::value, CR = decltype(cr)::value;
      // small batches (up to one wave per SIMD): 256-env tiles put a workgroup on every CU at 65,536 envs
      // and shorten its table staging: 6.75 us against 7.24 us per step there; 5 % slower at 131,072 envs, 1 % at
      // 1 Mi envs and beyond (profiles/r03_experiments/small_batch_variants.txt)
      if constexpr (CR == 10 && step_block<W>() > 256) {
        if (p.B <= kSmallBatch) {
          hipLaunchKernelGGL((step_kernel<W, C, NCH, CR, 256>), dim3((p.B + 255) / 256), dim3(256), 0, s, p);
          return;
        }
      }
      hipLaunchKernelGGL((step_kernel<W, C, NCH, CR>), step_grid<W>(p.B), dim3(step_block<W>()), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchStepMany {
  static void run(const StepManyParams& q, hipStream_t s) {
    tet::kernel_variant<W>(q.one.cfg.R, [&](auto nch, auto cr, auto) {
      constexpr int NCH = decltype(nch)::value, CR = decltype(cr)::value;
      if (q.policy == 1)  // the greedy policy evaluates terminal afterstates too: the afterstate family's tables
        hipLaunchKernelGGL((step_many_kernel<W, C, NCH, 1, 12>), step_grid<W>(q.one.B), dim3(step_block<W>()), 0, s, q);
      else
        hipLaunchKernelGGL((step_many_kernel<W, C, NCH, 0, CR>), step_grid<W>(q.one.B), dim3(step_block<W>()), 0, s, q);
    });
  }
};
template <typename W, int C>
struct LaunchReset {
  static void run(const ResetParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.R, [&](auto, auto, auto pack) {
      hipLaunchKernelGGL((reset_kernel<W, C, decltype(pack)::value>), grid_for(p.B), dim3(kBlock), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchRefresh {
  static void run(const RefreshParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.R, [&](auto, auto, auto pack) {
      hipLaunchKernelGGL((refresh_kernel<W, C, decltype(pack)::value>), grid_for(p.B), dim3(kBlock), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchRollouts {
  static void run(const RolloutParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.R, [&](auto nch, auto, auto) {
      hipLaunchKernelGGL((rollouts_kernel<W, C, decltype(nch)::value>), rollout_grid(p.B * p.a_max), dim3(kRolloutBlock), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchGreedy {
  static void run(const GreedyParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.R, [&](auto nch, auto, auto) {
      hipLaunchKernelGGL((greedy_kernel<W, C, decltype(nch)::value>), grid_for(p.B), dim3(kBlock), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchGreedyRows {
  static void run(const GreedyRowsParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.R, [&](auto nch, auto, auto) {
      hipLaunchKernelGGL((greedy_rows_kernel<W, C, decltype(nch)::value>), grid_for(p.B), dim3(kBlock), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchPlay {
  static void run(const PlayParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.cfg.R, [&](auto nch, auto, auto) {
      hipLaunchKernelGGL((play_linear_kernel<W, C, decltype(nch)::value>), step_grid<W>(p.B), dim3(step_block<W>()), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchSoftmaxRows {
  static void run(const SoftmaxRowsParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.R, [&](auto nch, auto, auto) {
      hipLaunchKernelGGL((softmax_rows_kernel<W, C, decltype(nch)::value>), grid_for(p.B), dim3(kBlock), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchPlaySoftmax {
  static void run(const PlaySoftmaxParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.play.cfg.R, [&](auto nch, auto, auto) {
      hipLaunchKernelGGL((play_softmax_kernel<W, C, decltype(nch)::value>), step_grid<W>(p.play.B), dim3(step_block<W>()), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchAfter {
  static void run(const AfterParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.R, [&](auto nch, auto, auto) {
      hipLaunchKernelGGL((afterstates_kernel<W, C, decltype(nch)::value>), grid_for(p.B), dim3(kBlock), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchExpand {
  static void run(const ExpandParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.cfg.R, [&](auto nch, auto cr, auto pack) {
      hipLaunchKernelGGL((expand_kernel<W, C, decltype(nch)::value, decltype(cr)::value, decltype(pack)::value>), grid_for(p.B_dst),
                         dim3(kBlock), 0, s, p);
    });
  }
};
template <typename W, int C>
struct LaunchTwoPly {
  static void run(const TwoPlyParams& p, hipStream_t s) {
    tet::kernel_variant<W>(p.R, [&](auto nch, auto, auto) {
      const int64_t epb = kRolloutBlock / p.a_max;  // whole envs per workgroup
      hipLaunchKernelGGL((two_ply_kernel<W, C, decltype(nch)::value>), dim3((unsigned)((p.B + epb - 1) / epb)), dim3(kRolloutBlock), 0, s, p);
    });
  }
};

template <> struct LaunchId<LaunchStep> { static constexpr int value = 0; };
template <> struct LaunchId<LaunchStepMany> { static constexpr int value = 1; };
template <> struct LaunchId<LaunchReset> { static constexpr int value = 2; };
template <> struct LaunchId<LaunchRefresh> { static constexpr int value = 3; };
template <> struct LaunchId<LaunchRollouts> { static constexpr int value = 4; };
template <> struct LaunchId<LaunchGreedy> { static constexpr int value = 5; };
template <> struct LaunchId<LaunchAfter> { static constexpr int value = 6; };
template <> struct LaunchId<LaunchGreedyRows> { static constexpr int value = 7; };
template <> struct LaunchId<LaunchPlay> { static constexpr int value = 8; };
template <> struct LaunchId<LaunchSoftmaxRows> { static constexpr int value = 9; };
template <> struct LaunchId<LaunchPlaySoftmax> { static constexpr int value = 10; };
template <> struct LaunchId<LaunchExpand> { static constexpr int value = 11; };
template <> struct LaunchId<LaunchTwoPly> { static constexpr int value = 12; };

template <template <typename, int> class Launcher, int CC, typename P>
inline void launch_words(int word_bytes, const void* p, hipStream_t s) {
  if (word_bytes == 4) Launcher<uint32_t, CC>::run(*static_cast<const P*>(p), s);
  else Launcher<uint64_t, CC>::run(*static_cast<const P*>(p), s);
}
// every launch of column count CC (instantiates all its kernels)
template <int CC>
int launch_part(int which, int word_bytes, const void* p, hipStream_t s) {
  switch (which) {
    case 0: launch_words<LaunchStep, CC, StepParams>(word_bytes, p, s); break;
    case 1: launch_words<LaunchStepMany, CC, StepManyParams>(word_bytes, p, s); break;
    case 2: launch_words<LaunchReset, CC, ResetParams>(word_bytes, p, s); break;
    case 3: launch_words<LaunchRefresh, CC, RefreshParams>(word_bytes, p, s); break;
    case 4: launch_words<LaunchRollouts, CC, RolloutParams>(word_bytes, p, s); break;
    case 5: launch_words<LaunchGreedy, CC, GreedyParams>(word_bytes, p, s); break;
    case 6: launch_words<LaunchAfter, CC, AfterParams>(word_bytes, p, s); break;
    case 7: launch_words<LaunchGreedyRows, CC, GreedyRowsParams>(word_bytes, p, s); break;
    case 8: launch_words<LaunchPlay, CC, PlayParams>(word_bytes, p, s); break;
    case 9: launch_words<LaunchSoftmaxRows, CC, SoftmaxRowsParams>(word_bytes, p, s); break;
    case 10: launch_words<LaunchPlaySoftmax, CC, PlaySoftmaxParams>(word_bytes, p, s); break;
    case 11: launch_words<LaunchExpand, CC, ExpandParams>(word_bytes, p, s); break;
    case 12: launch_words<LaunchTwoPly, CC, TwoPlyParams>(word_bytes, p, s); break;
    default: return TETRIS_E_DESC;
  }
  return (int)hipGetLastError();
}

}  // namespace

#if defined(TET_PART)
#define TET_PART_NAME2(c) tetris_part_##c
#define TET_PART_NAME(c) TET_PART_NAME2(c)
extern "C" __attribute__((visibility("hidden"))) int TET_PART_NAME(TET_PART)(int which, int word_bytes, const void* p,
                                                                            hipStream_t s) {
  return launch_part<TET_PART>(which, word_bytes, p, s);
}
#elif defined(TET_SPLIT_MAIN)
#define X(CC) extern "C" __attribute__((visibility("hidden"))) int tetris_part_##CC(int, int, const void*, hipStream_t);
TET_COLUMNS(X)
#undef X
#endif

namespace {

template <template <typename, int> class Launcher, typename P>
int dispatch(const TetrisDesc* d, const P& p, hipStream_t s) {
  switch (d->num_columns) {
#if defined(TET_SPLIT_MAIN)
#define X(CC) case CC: return tetris_part_##CC(LaunchId<Launcher>::value, d->word_bytes, &p, s);
#else
#define X(CC) case CC: return launch_part<CC>(LaunchId<Launcher>::value, d->word_bytes, &p, s);
#endif
    TET_COLUMNS(X)
#undef X
    default:
      return TETRIS_E_COLUMNS;
  }
}

}  // namespace

#if !defined(TET_PART)
// ---- C-ABI ---------------------------------------------------------------------------
// The text of the C-ABI is tetris_abi.inc, shared with the CPU harness; this is the backend it runs on here.
#ifndef TET_SRC_HASH
#define TET_SRC_HASH "unknown"
#endif
namespace {
namespace backend {

constexpr const char* kSourceHash = TET_SRC_HASH;
const char* error_text(int code) { return hipGetErrorString((hipError_t)code); }

int launch(const TetrisDesc* d, const StepParams& p, void* s) { return dispatch<LaunchStep>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const StepManyParams& p, void* s) { return dispatch<LaunchStepMany>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const ResetParams& p, void* s) { return dispatch<LaunchReset>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const RefreshParams& p, void* s) { return dispatch<LaunchRefresh>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const AfterParams& p, void* s) { return dispatch<LaunchAfter>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const GreedyParams& p, void* s) { return dispatch<LaunchGreedy>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const RolloutParams& p, void* s) { return dispatch<LaunchRollouts>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const GreedyRowsParams& p, void* s) { return dispatch<LaunchGreedyRows>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const PlayParams& p, void* s) { return dispatch<LaunchPlay>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const SoftmaxRowsParams& p, void* s) { return dispatch<LaunchSoftmaxRows>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const PlaySoftmaxParams& p, void* s) { return dispatch<LaunchPlaySoftmax>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const ExpandParams& p, void* s) { return dispatch<LaunchExpand>(d, p, (hipStream_t)s); }
int launch(const TetrisDesc* d, const TwoPlyParams& p, void* s) { return dispatch<LaunchTwoPly>(d, p, (hipStream_t)s); }

int launch(const TetrisDesc* d, const GatherParams& p, void* s) {  // one kernel per word size and plane count, whatever the columns
  const bool known = tet::gather_variant(p.n_planes, [&](auto np) {
    constexpr int NP = decltype(np)::value;
    if (d->word_bytes == 4) hipLaunchKernelGGL((gather_envs_kernel<uint32_t, NP>), grid_for(p.B_dst), dim3(kBlock), 0, (hipStream_t)s, p);
    else hipLaunchKernelGGL((gather_envs_kernel<uint64_t, NP>), grid_for(p.B_dst), dim3(kBlock), 0, (hipStream_t)s, p);
  });
  return known ? (int)hipGetLastError() : TETRIS_E_COLUMNS;
}

int stream_link(void* from_stream, void* to_stream) {
  // The event releases to DEVICE scope: producer and consumer run on the same GPU (the consumer is the RCCL
  // kernel that reads the gather payload), so the system-scope cache write-back a default event carries is
  // not needed -- that write-back is what made a recorded event cost the stepping stream tens of microseconds.
  hipEvent_t ev;
  hipError_t rc = hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventReleaseToDevice);
  if (rc != hipSuccess) return (int)rc;
  rc = hipEventRecord(ev, (hipStream_t)from_stream);
  if (rc == hipSuccess) rc = hipStreamWaitEvent((hipStream_t)to_stream, ev, 0);
  const hipError_t rc2 = hipEventDestroy(ev);  // (released once the wait has consumed it)
  return (int)(rc != hipSuccess ? rc : rc2);
}

int pack_done_bits(const uint8_t* done, uint8_t* bits, int64_t B, void* s) {
  hipLaunchKernelGGL(pack_done_bits_kernel, grid_for(B), dim3(kBlock), 0, (hipStream_t)s, done,
                     reinterpret_cast<unsigned long long*>(bits), B);
  return (int)hipGetLastError();
}

int counter_add(uint64_t* counter, uint64_t n, void* s) {
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, counter, n);
  return (int)hipGetLastError();
}

int policy_random(const uint8_t* n_valid, int32_t* action, uint32_t key, int64_t env_offset, int64_t B, void* s) {
  hipLaunchKernelGGL(policy_random_kernel, grid_for(B), dim3(kBlock), 0, (hipStream_t)s, n_valid, action, key,
                     env_offset, B);
  return (int)hipGetLastError();
}

int numpy_bag_stream(const uint32_t* seeds, int32_t n_pieces, int64_t L, uint8_t* stream, int64_t B, void* s) {
  hipLaunchKernelGGL(numpy_bag_stream_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)s, seeds,
                     n_pieces, L, stream, B);
  return (int)hipGetLastError();
}

int decode(int word_bytes, const void* cols, int8_t* cells, int32_t* heights, int C, int rows, int64_t B,
                  bool packed, void* s) {
  if (word_bytes == 4)
    hipLaunchKernelGGL((decode_kernel<uint32_t>), grid_for(B), dim3(kBlock), 0, (hipStream_t)s,
                       static_cast<const uint32_t*>(cols), cells, heights, C, rows, B, packed);
  else
    hipLaunchKernelGGL((decode_kernel<uint64_t>), grid_for(B), dim3(kBlock), 0, (hipStream_t)s,
                       static_cast<const uint64_t*>(cols), cells, heights, C, rows, B, packed);
  return (int)hipGetLastError();
}

int encode(int word_bytes, const int8_t* cells, void* cols, int C, int rows, int64_t B, bool packed, void* s) {
  if (word_bytes == 4)
    hipLaunchKernelGGL((encode_kernel<uint32_t>), grid_for(B), dim3(kBlock), 0, (hipStream_t)s, cells,
                       static_cast<uint32_t*>(cols), C, rows, B, packed);
  else
    hipLaunchKernelGGL((encode_kernel<uint64_t>), grid_for(B), dim3(kBlock), 0, (hipStream_t)s, cells,
                       static_cast<uint64_t*>(cols), C, rows, B, packed);
  return (int)hipGetLastError();
}

}  // namespace backend
}  // namespace

#define TET_ABI(name) tetris_hip_##name
#include "tetris_abi.inc"

#if TET_STAMPS
extern "C" int tetris_debug_read_stamps(uint64_t* dst, int n_wgs) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps), sizeof(uint64_t) * kStampWords * (size_t)n_wgs, 0,
                                  hipMemcpyDeviceToHost);
}
#endif
#endif  // !TET_PART
