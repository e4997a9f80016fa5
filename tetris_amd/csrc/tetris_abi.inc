// tetris_abi.inc -- the C-ABI of include/tetris_hip.h, written once: every argument check and its error code,
// every key derivation and the filling of every parameter block (tetris_entry.hpp).  tetris_kernels.hip includes
// it for libtetris_hip.so, tests/harness/core_host.cpp for the CPU harness.  The includer defines
//   TET_ABI(name)       the exported symbol: tetris_hip_##name / tetris_host_##name
//   namespace backend   what differs between a GPU and a loop over envs, each returning an error code:
//     launch(const TetrisDesc*, const XParams&, void* stream), overloaded on the parameter blocks (the CPU harness
//     takes those of the gather, population, softmax, expand and two-ply calls from tetris_entry.hpp);
//     pack_done_bits, counter_add, policy_random, numpy_bag_stream, decode, encode, stream_link (the arguments
//     below); error_text(code) for a positive (runtime) code; kSourceHash.
// Nothing here launches or touches a buffer: a refused call returns before the backend is reached.

namespace {

// a batch of B envs (max_elems per-step output elements) whose kernels may address it with 32-bit byte offsets:
// every output offset (<= 32 B/element) and every board record
bool batch_fits_u32_offsets(int64_t B, int64_t max_elems) {
  return max_elems <= 0x7FFFFFFF / 32 && (B + 63) / 64 * 64 * (int64_t)tet::kMaxCols * 8 <= 0xFFFFFFFFll;
}

// a softmax temperature: positive and finite, and so is the 1.0f / temperature the kernels multiply by
bool softmax_temperature_ok(float t) { return t > 0.f && t <= 3.402823466e+38f && 1.0f / t <= 3.402823466e+38f; }

// two batches of one geometry share storage: the byte ranges of their cols or of their meta overlap
bool batches_overlap(const TetrisDesc* desc, int np, const void* src_cols, const uint64_t* src_meta, int64_t B_src,
                     const void* dst_cols, const uint64_t* dst_meta, int64_t B_dst) {
  auto overlap = [](const void* a, int64_t na, const void* b, int64_t nb) {  // byte ranges [a, a + na) and [b, b + nb)
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
  };
  return overlap(src_cols, desc->word_bytes * tet::board_words(B_src, np), dst_cols, desc->word_bytes * tet::board_words(B_dst, np)) ||
         overlap(src_meta, 8 * B_src, dst_meta, 8 * B_dst);
}

int fill_step_params(StepParams& p, const TetrisDesc* desc, void* cols, uint64_t* meta, const int32_t* action,
                     int32_t* action_out, const uint8_t* stream, int32_t* cursor, int64_t stream_len, float* obs,
                     int32_t* reward, uint8_t* done, uint8_t* lines, uint8_t* n_valid_next, uint8_t* piece_next,
                     uint32_t* status, int32_t auto_reset, uint64_t seed, uint64_t step_idx, int64_t env_offset,
                     int64_t B, int64_t max_elems) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta || !reward || !done || !lines || !n_valid_next) return TETRIS_E_NULL;
  if (B <= 0 || !batch_fits_u32_offsets(B, max_elems)) return TETRIS_E_BATCH;
  if (stream && (!cursor || stream_len <= 0)) return TETRIS_E_STREAM;
  p.cols = cols;
  p.meta = meta;
  p.action = action;
  p.action_out = action_out;
  p.stream = stream;
  p.cursor = cursor;
  p.stream_len = stream_len;
  p.obs = obs;
  p.reward = reward;
  p.done = done;
  p.lines = lines;
  p.n_valid = n_valid_next;
  p.piece_next = piece_next;
  p.status = status;
  p.done_bits = nullptr;        // (the gather payload is attached per call: step_call_run_gather)
  p.status_snapshot = nullptr;
  p.B = (uint32_t)B;
  p.env_offset = (uint32_t)env_offset;
  p.step_counter = nullptr;
  p.seed = seed;
  p.step_rel = 0;
  tet::fill_step_cfg(p.cfg, desc, auto_reset, obs != nullptr);
  tet::step_keys(seed, step_idx, p.cfg);
  tet::build_table(desc, &p.tab);
  return TETRIS_OK;
}

// what the three runs of a bound call share: the checks, then this step's action / action_out and keys into the
// bound parameters
int step_call_begin(void* call_, const int32_t* action, uint64_t step_idx, TetrisStepCall*& call) {
  call = static_cast<TetrisStepCall*>(call_);
  if (!call) return TETRIS_E_NULL;
  if (call->magic != kStepCallMagic) return TETRIS_E_DESC;
  call->p.action = action;
  call->p.action_out = action ? nullptr : call->action_out;
  tet::step_keys(call->seed, step_idx, call->p.cfg);
  return TETRIS_OK;
}

}  // namespace

extern "C" {

int TET_ABI(version)(void) { return TETRIS_HIP_ABI_VERSION; }

const char* TET_ABI(error_string)(int code) {
  const char* own = tet::error_text(code);
  return own ? own : (code > 0 ? backend::error_text(code) : "unknown error");
}

const char* TET_ABI(source_hash)(void) { return backend::kSourceHash; }

int TET_ABI(supported_columns)(int32_t* out, int cap) {
  int n = 0;
#define X(CC) if (out && n < cap) out[n] = CC; ++n;
  TET_COLUMNS(X)
#undef X
  return n;
}

int TET_ABI(n_planes)(const TetrisDesc* desc) {
  const int rc = tet::check_desc(desc);
  if (rc) return rc;
  return tet::n_planes(desc->num_columns, tet::board_packed(desc->word_bytes, desc->num_rows));
}

int64_t TET_ABI(board_words)(const TetrisDesc* desc, int64_t B) {
  const int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (B <= 0) return TETRIS_E_BATCH;
  return tet::board_words(B, tet::n_planes(desc->num_columns, tet::board_packed(desc->word_bytes, desc->num_rows)));
}

int64_t TET_ABI(status_words)(int64_t B) {
  if (B <= 0) return 0;
  // one 16-byte slot per wavefront, rounded up to the largest tile a stepping kernel may use
  return 4 * (((B + 1023) / 1024) * 16);
}

int TET_ABI(n_placements)(int32_t catalogue_id, int32_t num_columns) {
  if (catalogue_id < 0 || catalogue_id >= TETRIS_N_CATALOGUE) return TETRIS_E_PIECES;
  return tet::n_placements(catalogue_id, num_columns);
}

int TET_ABI(desc_init)(TetrisDesc* desc, int32_t num_columns, int32_t num_rows, const int32_t* piece_ids,
                       int32_t n_pieces, const float* direct_by) {
  return tet::desc_init(desc, num_columns, num_rows, piece_ids, n_pieces, direct_by);
}

int TET_ABI(reset)(const TetrisDesc* desc, void* cols, uint64_t* meta, const uint8_t* reset_mask, uint8_t* piece_out,
                   uint8_t* n_valid_out, const uint8_t* stream, int32_t* cursor, int64_t stream_len, uint32_t* status,
                   int32_t init_bag, uint64_t seed, uint64_t step_idx, int64_t env_offset, int64_t B,
                   void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta) return TETRIS_E_NULL;
  if (B <= 0) return TETRIS_E_BATCH;
  if (stream && (!cursor || stream_len <= 0)) return TETRIS_E_STREAM;
  ResetParams p{};
  p.cols = cols;
  p.meta = meta;
  p.status = status;
  p.reset_mask = reset_mask;
  p.piece_out = piece_out;
  p.n_valid_out = n_valid_out;
  p.stream = stream;
  p.cursor = cursor;
  p.stream_len = stream_len;
  p.B = B;
  p.env_offset = env_offset;
  p.init_bag = init_bag;
  p.n_pieces = desc->n_pieces;
  p.R = desc->num_rows;
  p.key = tet::hash_key(seed, step_idx * 4u + 2u);
  tet::build_table(desc, &p.tab);
  return backend::launch(desc, p, hip_stream);
}

int TET_ABI(step_many)(const TetrisDesc* desc, void* cols, uint64_t* meta, int32_t n_steps, int32_t policy,
                       const float* weights, int32_t* action_out, float* obs, int32_t* reward, uint8_t* done,
                       uint8_t* lines, uint8_t* n_valid_next, uint8_t* piece_next, uint32_t* status,
                       int32_t auto_reset, uint64_t seed, uint64_t step_idx0, int64_t env_offset, int64_t B,
                       void* hip_stream) {
  if (n_steps < 1 || policy < 0 || policy > 1 || (policy == 1 && !weights)) return TETRIS_E_BATCH;
  StepManyParams q{};
  int rc = fill_step_params(q.one, desc, cols, meta, nullptr, action_out, nullptr, nullptr, 0, obs, reward, done,
                            lines, n_valid_next, piece_next, status, auto_reset, seed, step_idx0, env_offset, B,
                            (int64_t)B * n_steps);
  if (rc) return rc;
  q.n_steps = n_steps;
  q.policy = policy;
  q.seed = seed;
  q.step_idx0 = step_idx0;
  for (int i = 0; i < 8; ++i) q.w[i] = weights ? weights[i] : 0.f;
  return backend::launch(desc, q, hip_stream);
}

int TET_ABI(step)(const TetrisDesc* desc, void* cols, uint64_t* meta, const int32_t* action, int32_t* action_out,
                  const uint8_t* stream, int32_t* cursor, int64_t stream_len, float* obs, int32_t* reward,
                  uint8_t* done, uint8_t* lines, uint8_t* n_valid_next, uint8_t* piece_next, uint32_t* status,
                  int32_t auto_reset, uint64_t seed, uint64_t step_idx, int64_t env_offset, int64_t B,
                  void* hip_stream) {
  StepParams p{};
  int rc = fill_step_params(p, desc, cols, meta, action, action_out, stream, cursor, stream_len, obs, reward, done,
                            lines, n_valid_next, piece_next, status, auto_reset, seed, step_idx, env_offset, B, B);
  if (rc) return rc;
  return backend::launch(desc, p, hip_stream);
}

// ---- bound step call (TetrisStepCall: tetris_entry.hpp) ---------------------------------------------
int64_t TET_ABI(step_call_size)(void) { return (int64_t)sizeof(TetrisStepCall); }

int TET_ABI(step_call_init)(void* call_, const TetrisDesc* desc, void* cols, uint64_t* meta, int32_t* action_out,
                            const uint8_t* stream, int32_t* cursor, int64_t stream_len, float* obs, int32_t* reward,
                            uint8_t* done, uint8_t* lines, uint8_t* n_valid_next, uint8_t* piece_next,
                            uint32_t* status, int32_t auto_reset, uint64_t seed, int64_t env_offset, int64_t B) {
  if (!call_) return TETRIS_E_NULL;
  TetrisStepCall* call = static_cast<TetrisStepCall*>(call_);
  call->magic = 0;
  int rc = fill_step_params(call->p, desc, cols, meta, nullptr, nullptr, stream, cursor, stream_len, obs, reward, done,
                            lines, n_valid_next, piece_next, status, auto_reset, seed, 0, env_offset, B, B);
  if (rc) return rc;
  call->desc = *desc;
  call->seed = seed;
  call->action_out = action_out;
  call->magic = kStepCallMagic;
  return TETRIS_OK;
}

int TET_ABI(step_call_run)(void* call_, const int32_t* action, uint64_t step_idx, void* hip_stream) {
  TetrisStepCall* call;
  const int rc = step_call_begin(call_, action, step_idx, call);
  if (rc) return rc;
  return backend::launch(&call->desc, call->p, hip_stream);
}

int TET_ABI(step_call_run_gather)(void* call_, const int32_t* action, uint64_t step_idx, uint64_t* done_bits,
                                  uint32_t* status_snapshot, void* hip_stream) {
  TetrisStepCall* call;
  const int rc = step_call_begin(call_, action, step_idx, call);
  if (rc) return rc;
  StepParams p = call->p;  // (a copy: the bound call itself stays free of the payload pointers)
  p.done_bits = reinterpret_cast<unsigned long long*>(done_bits);
  p.status_snapshot = status_snapshot;
  return backend::launch(&call->desc, p, hip_stream);
}

int TET_ABI(step_call_run_counted)(void* call_, const int32_t* action, const uint64_t* step_counter, uint32_t step_rel,
                                   void* hip_stream) {
  if (!step_counter) return TETRIS_E_NULL;
  TetrisStepCall* call;
  const int rc = step_call_begin(call_, action, 0, call);  // (the step derives the keys from the counter)
  if (rc) return rc;
  StepParams p = call->p;  // (a copy: the bound call itself stays usable for plain runs)
  p.step_counter = step_counter;
  p.step_rel = step_rel;
  return backend::launch(&call->desc, p, hip_stream);
}

// `to_stream` waits for everything enqueued on `from_stream` so far
int TET_ABI(stream_link)(void* from_stream, void* to_stream) { return backend::stream_link(from_stream, to_stream); }

int TET_ABI(pack_done_bits)(const uint8_t* done, uint8_t* bits, int64_t B, void* hip_stream) {
  if (!done || !bits) return TETRIS_E_NULL;
  if (B <= 0) return TETRIS_E_BATCH;
  return backend::pack_done_bits(done, bits, B, hip_stream);
}

int TET_ABI(counter_add)(uint64_t* counter, uint64_t n, void* hip_stream) {
  if (!counter) return TETRIS_E_NULL;
  return backend::counter_add(counter, n, hip_stream);
}

int TET_ABI(afterstates)(const TetrisDesc* desc, const void* cols, const uint64_t* meta, float* feats,
                         uint8_t* n_valid, float* feats_all, uint8_t* n_all, int64_t env_stride, int64_t row_stride,
                         int64_t B, void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta || !feats || !n_valid) return TETRIS_E_NULL;
  if (B <= 0) return TETRIS_E_BATCH;
  if (env_stride % 4 || row_stride % 4 || env_stride < 8 || row_stride < 8) return TETRIS_E_STRIDE;
  // the kernel addresses rows with 32-bit float4 indices
  if ((B - 1) * (env_stride / 4) + (int64_t)(desc->a_max - 1) * (row_stride / 4) + 2 >= 0xFFFFFFFFll) return TETRIS_E_STRIDE;
  AfterParams p{};
  p.cols = cols;
  p.meta = meta;
  p.feats = feats;
  p.n_valid = n_valid;
  p.feats_all = feats_all;
  p.n_all = n_all;
  p.B = B;
  p.env_stride = env_stride;
  p.row_stride = row_stride;
  p.R = desc->num_rows;
  p.a_max = desc->a_max;
  p.has_direct_by = desc->has_direct_by;
  for (int i = 0; i < 8; ++i) p.direct_by[i] = desc->direct_by[i];
  tet::build_table(desc, &p.tab);
  return backend::launch(desc, p, hip_stream);
}

int TET_ABI(policy_greedy)(const TetrisDesc* desc, const void* cols, const uint64_t* meta, const float* weights,
                           int32_t* best_action, float* best_value, float* fitness_all, int64_t B,
                           void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta || !weights || !best_action) return TETRIS_E_NULL;
  if (B <= 0) return TETRIS_E_BATCH;
  GreedyParams p{};
  p.cols = cols;
  p.meta = meta;
  p.best_action = best_action;
  p.best_value = best_value;
  p.fitness_all = fitness_all;
  p.B = B;
  p.R = desc->num_rows;
  p.a_max = desc->a_max;
  for (int i = 0; i < 8; ++i) p.w[i] = weights[i];
  tet::build_table(desc, &p.tab);
  return backend::launch(desc, p, hip_stream);
}

// policy_greedy with the weight row taken per env from a DEVICE matrix weights[P][8]
int TET_ABI(policy_greedy_rows)(const TetrisDesc* desc, const void* cols, const uint64_t* meta, const float* weights,
                                int32_t P, const int32_t* rows, int32_t* best_action, float* best_value,
                                uint32_t* status, int64_t B, void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta || !weights || !best_action) return TETRIS_E_NULL;
  if (B <= 0 || !batch_fits_u32_offsets(B, B) || P < 1 || (!rows && P < B)) return TETRIS_E_BATCH;
  GreedyRowsParams p{};
  p.cols = cols;
  p.meta = meta;
  p.weights = weights;
  p.rows = rows;
  p.best_action = best_action;
  p.best_value = best_value;
  p.status = status;
  p.B = B;
  p.P = P;
  p.R = desc->num_rows;
  tet::build_table(desc, &p.tab);
  return backend::launch(desc, p, hip_stream);
}

// n_steps greedy steps of every env on its own weight row in one launch: no auto-reset, an env that is over is
// frozen; per-env totals instead of a trajectory
int TET_ABI(play_linear)(const TetrisDesc* desc, void* cols, uint64_t* meta, int32_t n_steps, const float* weights,
                         int32_t P, const int32_t* rows, uint32_t* lines_total, uint32_t* pieces_total,
                         uint8_t* n_valid, uint8_t* piece, uint32_t* status, uint64_t seed, uint64_t step_idx0,
                         int64_t env_offset, int64_t B, void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta || !weights || !lines_total || !pieces_total) return TETRIS_E_NULL;
  if (B <= 0 || !batch_fits_u32_offsets(B, B) || n_steps < 1 || P < 1 || (!rows && P < B)) return TETRIS_E_BATCH;
  PlayParams p{};
  p.cols = cols;
  p.meta = meta;
  p.weights = weights;
  p.rows = rows;
  p.lines_total = lines_total;
  p.pieces_total = pieces_total;
  p.n_valid = n_valid;
  p.piece = piece;
  p.status = status;
  p.B = (uint32_t)B;
  p.env_offset = (uint32_t)env_offset;
  p.P = P;
  p.n_steps = n_steps;
  p.seed = seed;
  p.step_idx0 = step_idx0;
  tet::fill_step_cfg(p.cfg, desc, 0, false);  // never resets; no observation is written
  tet::step_keys(seed, step_idx0, p.cfg);
  tet::build_table(desc, &p.tab);
  return backend::launch(desc, p, hip_stream);
}

// one sampled decision per env from the softmax of its weight row's logits, with log-probability and score
int TET_ABI(policy_softmax_rows)(const TetrisDesc* desc, const void* cols, const uint64_t* meta, const float* weights,
                                 int32_t P, const int32_t* rows, float temperature, int32_t* action, float* logp,
                                 float* score, float* logz, float* logits, uint32_t* status, uint64_t seed,
                                 uint64_t step_idx, int64_t env_offset, int64_t B, void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta || !weights || !action || !logp) return TETRIS_E_NULL;
  if (B <= 0 || !batch_fits_u32_offsets(B, B) || P < 1 || (!rows && P < B)) return TETRIS_E_BATCH;
  if (!softmax_temperature_ok(temperature)) return TETRIS_E_TEMPERATURE;
  if ((uintptr_t)weights % 16 || (uintptr_t)score % 16) return TETRIS_E_ALIGN;
  SoftmaxRowsParams p{};
  p.cols = cols;
  p.meta = meta;
  p.weights = weights;
  p.rows = rows;
  p.action = action;
  p.logp = logp;
  p.score = score;
  p.logz = logz;
  p.logits = logits;
  p.status = status;
  p.B = B;
  p.P = P;
  p.R = desc->num_rows;
  p.a_max = desc->a_max;
  p.has_direct_by = desc->has_direct_by;
  for (int i = 0; i < 8; ++i) p.direct_by[i] = desc->direct_by[i];
  p.inv_t = 1.0f / temperature;
  p.key = tet::softmax_key(seed, step_idx);
  p.env_offset = (uint32_t)env_offset;
  tet::build_table(desc, &p.tab);
  return backend::launch(desc, p, hip_stream);
}

// n_steps sampled steps of every env in one launch: tetris_hip_play_linear with the pick drawn from the softmax
int TET_ABI(play_softmax)(const TetrisDesc* desc, void* cols, uint64_t* meta, int32_t n_steps, const float* weights,
                          int32_t P, const int32_t* rows, float temperature, uint32_t* lines_total,
                          uint32_t* pieces_total, float* logp_total, float* score_total, uint8_t* n_valid,
                          uint8_t* piece, uint32_t* status, uint64_t seed, uint64_t step_idx0, int64_t env_offset,
                          int64_t B, void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta || !weights || !lines_total || !pieces_total || !score_total) return TETRIS_E_NULL;
  if (B <= 0 || !batch_fits_u32_offsets(B, B) || n_steps < 1 || P < 1 || (!rows && P < B)) return TETRIS_E_BATCH;
  if (!softmax_temperature_ok(temperature)) return TETRIS_E_TEMPERATURE;
  if ((uintptr_t)weights % 16 || (uintptr_t)score_total % 16) return TETRIS_E_ALIGN;
  PlaySoftmaxParams q{};
  PlayParams& p = q.play;
  p.cols = cols;
  p.meta = meta;
  p.weights = weights;
  p.rows = rows;
  p.lines_total = lines_total;
  p.pieces_total = pieces_total;
  p.n_valid = n_valid;
  p.piece = piece;
  p.status = status;
  p.B = (uint32_t)B;
  p.env_offset = (uint32_t)env_offset;
  p.P = P;
  p.n_steps = n_steps;
  p.seed = seed;
  p.step_idx0 = step_idx0;
  tet::fill_step_cfg(p.cfg, desc, 0, false);  // never resets; no observation is written (direct_by serves the logits)
  tet::step_keys(seed, step_idx0, p.cfg);
  tet::build_table(desc, &p.tab);
  q.logp_total = logp_total;
  q.score_total = score_total;
  q.inv_t = 1.0f / temperature;
  return backend::launch(desc, q, hip_stream);
}

int TET_ABI(rollouts)(const TetrisDesc* desc, const void* cols, const uint64_t* meta, double* returns, int32_t length,
                      int32_t n, int32_t policy, const float* weights, const uint8_t* pieces, uint64_t seed,
                      uint64_t step_idx, int64_t env_offset, int64_t B, void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta || !returns || (policy == 1 && !weights)) return TETRIS_E_NULL;
  if (B <= 0 || length < 1 || n < 1 || policy < 0 || policy > 1) return TETRIS_E_BATCH;
  RolloutParams p{};
  p.cols = cols;
  p.meta = meta;
  p.returns = returns;
  p.B = B;
  p.env_offset = env_offset;
  p.R = desc->num_rows;
  p.a_max = desc->a_max;
  p.n_pieces = desc->n_pieces;
  p.length = length;
  p.n = n;
  p.policy = policy;
  p.pieces = pieces;
  p.key = tet::hash_key(seed ^ 0x526F6C6C6F757473ull, step_idx);
  for (int i = 0; i < 8; ++i) p.w[i] = weights ? weights[i] : 0.f;
  tet::build_table(desc, &p.tab);
  return backend::launch(desc, p, hip_stream);
}

int TET_ABI(refresh)(const TetrisDesc* desc, const void* cols, uint64_t* meta, uint8_t* n_valid_out, int64_t B,
                     void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta) return TETRIS_E_NULL;
  if (B <= 0) return TETRIS_E_BATCH;
  RefreshParams p{};
  p.cols = cols;
  p.meta = meta;
  p.n_valid_out = n_valid_out;
  p.B = B;
  p.R = desc->num_rows;
  tet::build_table(desc, &p.tab);
  return backend::launch(desc, p, hip_stream);
}

// dst env j := src env index[j] (-1: keep); the two batches must not share storage
int TET_ABI(gather_envs)(const TetrisDesc* desc, const void* src_cols, const uint64_t* src_meta, int64_t B_src,
                         void* dst_cols, uint64_t* dst_meta, uint8_t* dst_n_valid, uint8_t* dst_piece,
                         const int32_t* index, uint32_t* status, int64_t B_dst, void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!src_cols || !src_meta || !dst_cols || !dst_meta || !index) return TETRIS_E_NULL;
  if (B_src <= 0 || B_dst <= 0 || !batch_fits_u32_offsets(B_src, B_src) || !batch_fits_u32_offsets(B_dst, B_dst))
    return TETRIS_E_BATCH;
  const int np = tet::n_planes(desc->num_columns, tet::board_packed(desc->word_bytes, desc->num_rows));
  if (batches_overlap(desc, np, src_cols, src_meta, B_src, dst_cols, dst_meta, B_dst)) return TETRIS_E_OVERLAP;
  GatherParams p{};
  p.src_cols = src_cols;
  p.src_meta = src_meta;
  p.dst_cols = dst_cols;
  p.dst_meta = dst_meta;
  p.dst_n_valid = dst_n_valid;
  p.dst_piece = dst_piece;
  p.index = index;
  p.status = status;
  p.B_src = B_src;
  p.B_dst = B_dst;
  p.n_planes = np;
  tet::SetTable tab;
  tet::build_table(desc, &tab);
  for (int i = 0; i < desc->n_pieces; ++i) p.fullmask[i] = tab.fullmask[i];
  return backend::launch(desc, p, hip_stream);
}

// dst env j := src env parent[j] after placement action[j], the next piece dictated or drawn from the parent's bag
int TET_ABI(expand_envs)(const TetrisDesc* desc, const void* src_cols, const uint64_t* src_meta, int64_t B_src,
                         void* dst_cols, uint64_t* dst_meta, const int32_t* parent, const int32_t* action,
                         const uint8_t* next_piece, float* obs, int32_t* reward, uint8_t* done, uint8_t* lines,
                         uint8_t* n_valid, uint8_t* piece, uint32_t* status, uint64_t seed, uint64_t step_idx,
                         int64_t env_offset, int64_t B_dst, void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!src_cols || !src_meta || !dst_cols || !dst_meta || !parent || !action || !reward || !done || !lines || !n_valid || !piece)
    return TETRIS_E_NULL;
  if (B_src <= 0 || B_dst <= 0 || !batch_fits_u32_offsets(B_src, B_src) || !batch_fits_u32_offsets(B_dst, B_dst))
    return TETRIS_E_BATCH;
  const int np = tet::n_planes(desc->num_columns, tet::board_packed(desc->word_bytes, desc->num_rows));
  if (batches_overlap(desc, np, src_cols, src_meta, B_src, dst_cols, dst_meta, B_dst)) return TETRIS_E_OVERLAP;
  ExpandParams p{};
  p.src_cols = src_cols;
  p.src_meta = src_meta;
  p.dst_cols = dst_cols;
  p.dst_meta = dst_meta;
  p.parent = parent;
  p.action = action;
  p.next_piece = next_piece;
  p.obs = obs;
  p.reward = reward;
  p.done = done;
  p.lines = lines;
  p.n_valid = n_valid;
  p.piece = piece;
  p.status = status;
  p.B_src = (uint32_t)B_src;
  p.B_dst = (uint32_t)B_dst;
  p.env_offset = (uint32_t)env_offset;
  tet::fill_step_cfg(p.cfg, desc, 0, obs != nullptr);  // never resets: a child that is over keeps its board
  tet::step_keys(seed, step_idx, p.cfg);
  tet::build_table(desc, &p.tab);
  return backend::launch(desc, p, hip_stream);
}

// two-piece lookahead: the value of every (first action, next piece), its sum over the env's bag and the best action
int TET_ABI(policy_two_ply)(const TetrisDesc* desc, const void* cols, const uint64_t* meta, const float* weights,
                            float death_value, float* values, float* q, uint8_t* n_bag, int32_t* best_action,
                            float* best_value, int64_t B, void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !meta || !weights) return TETRIS_E_NULL;
  if (B <= 0 || !batch_fits_u32_offsets(B, B)) return TETRIS_E_BATCH;
  if (!(death_value <= 3.402823466e+38f)) return TETRIS_E_VALUE;  // NaN, +inf
  if (!values && !q && !n_bag && !best_action && !best_value) return TETRIS_OK;  // nothing asked for
  TwoPlyParams p{};
  p.cols = cols;
  p.meta = meta;
  p.values = values;
  p.q = q;
  p.n_bag = n_bag;
  p.best_action = best_action;
  p.best_value = best_value;
  p.B = B;
  p.R = desc->num_rows;
  p.a_max = desc->a_max;
  p.n_pieces = desc->n_pieces;
  p.death_value = death_value;
  for (int i = 0; i < 8; ++i) p.w[i] = weights[i];
  tet::build_table(desc, &p.tab);
  return backend::launch(desc, p, hip_stream);
}

int TET_ABI(policy_random)(const uint8_t* n_valid, int32_t* action, uint64_t seed, uint64_t step_idx,
                           int64_t env_offset, int64_t B, void* hip_stream) {
  if (!n_valid || !action) return TETRIS_E_NULL;
  if (B <= 0) return TETRIS_E_BATCH;
  return backend::policy_random(n_valid, action, tet::hash_key(seed, step_idx * 4u + 3u), env_offset, B, hip_stream);
}

int TET_ABI(numpy_bag_stream)(const uint32_t* seeds, int32_t n_pieces, int64_t L, uint8_t* stream, int64_t B,
                              void* hip_stream) {
  if (!seeds || !stream) return TETRIS_E_NULL;
  if (n_pieces < 1 || n_pieces > TETRIS_MAX_PIECES) return TETRIS_E_PIECES;
  if (B <= 0 || L <= 0) return TETRIS_E_BATCH;
  return backend::numpy_bag_stream(seeds, n_pieces, L, stream, B, hip_stream);
}

// cells [B][rows][C] <-> stored boards; rows = num_rows + 4
int TET_ABI(decode)(const TetrisDesc* desc, const void* cols, int8_t* cells, int32_t* heights, int64_t B,
                    void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols) return TETRIS_E_NULL;
  if (B <= 0) return TETRIS_E_BATCH;
  return backend::decode(desc->word_bytes, cols, cells, heights, desc->num_columns, desc->num_rows + 4, B,
                         tet::board_packed(desc->word_bytes, desc->num_rows), hip_stream);
}

int TET_ABI(encode)(const TetrisDesc* desc, const int8_t* cells, void* cols, int64_t B, void* hip_stream) {
  int rc = tet::check_desc(desc);
  if (rc) return rc;
  if (!cols || !cells) return TETRIS_E_NULL;
  if (B <= 0) return TETRIS_E_BATCH;
  return backend::encode(desc->word_bytes, cells, cols, desc->num_columns, desc->num_rows + 4, B,
                         tet::board_packed(desc->word_bytes, desc->num_rows), hip_stream);
}

}  // extern "C"
