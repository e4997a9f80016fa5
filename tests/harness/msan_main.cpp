// MemorySanitizer driver for the per-lane logic (CPU only; not part of the test suite):
//   /opt/rocm/lib/llvm/bin/clang++ -fsanitize=memory -fsanitize-memory-track-origins -O1 -g -std=c++17 msan_main.cpp -o msan_main
// (or g++ -fsanitize=address,undefined -fno-sanitize-recover=undefined -O1 -g -std=c++17 msan_main.cpp -o asan_main)
// Runs every entry of the afterstate family on boards of several widths, then the text of the C-ABI
// (tetris_abi.inc): calls it must refuse and the bound step call; any use of an uninitialised value in a
// branch, address or output is reported.
#include "core_host.cpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int run(int C, int R, const std::vector<int32_t>& ids, int64_t B) {
  TetrisDesc d;
  memset(&d, 0, sizeof d);
  if (tetris_host_desc_init(&d, C, R, ids.data(), (int32_t)ids.size(), nullptr) != 0) return 1;
  const int64_t words = tetris_host_board_words(&d, B);
  std::vector<uint64_t> cols(words + 8, 0), meta(B, 0);
  std::vector<uint8_t> piece(B, 0), nv(B, 0), done(B * 40, 0), lines(B * 40, 0), nvn(B * 40, 0), pn(B * 40, 0);
  std::vector<uint32_t> status(tetris_host_status_words(B) + 16, 0);
  std::vector<int32_t> act(B * 40, 0), rew(B * 40, 0);
  std::vector<float> obs(B * 40 * 8, 0.f);
  const float w[8] = {-12.63f, 6.60f, -9.22f, -19.77f, -13.08f, -10.49f, -1.61f, -24.04f};
  int rc = tetris_host_reset(&d, cols.data(), meta.data(), nullptr, piece.data(), nv.data(), nullptr, nullptr, 0, status.data(), 1,
                             7, 0, 0, B, nullptr);
  rc |= tetris_host_step_many(&d, cols.data(), meta.data(), 30, 0, w, act.data(), obs.data(), rew.data(), done.data(), lines.data(),
                              nvn.data(), pn.data(), status.data(), 1, 7, 0, 0, B, nullptr);
  const int A = d.a_max;
  std::vector<float> feats(B * A * 8, 0.f), feats_all(B * A * 8, 0.f), fit(B * A, 0.f), bv(B, 0.f);
  std::vector<uint8_t> n1(B, 0), n2(B, 0);
  std::vector<int32_t> ba(B, 0);
  std::vector<double> ret(B * A, 0.0);
  rc |= tetris_host_afterstates(&d, cols.data(), meta.data(), feats.data(), n1.data(), feats_all.data(), n2.data(), A * 8, 8, B, nullptr);
  rc |= tetris_host_policy_greedy(&d, cols.data(), meta.data(), w, ba.data(), bv.data(), fit.data(), B, nullptr);
  rc |= tetris_host_rollouts(&d, cols.data(), meta.data(), ret.data(), 3, 2, 1, w, nullptr, 7, 30, 0, B, nullptr);
  rc |= tetris_host_step_many(&d, cols.data(), meta.data(), 6, 1, w, act.data(), obs.data(), rew.data(), done.data(), lines.data(),
                              nvn.data(), pn.data(), status.data(), 1, 7, 30, 0, B, nullptr);
  double s = 0;
  for (float x : fit) s += x;
  for (double x : ret) s += (x == x) ? x : 0;
  for (float x : feats_all) s += x;
  for (int32_t x : ba) s += x;
  printf("%2d x %2d, %zu pieces: rc %d checksum %.3f\n", C, R, ids.size(), rc, s);
  return rc;
}

// the bound call: init, run, run_gather, run_counted must play what three plain steps play
static int bound_call(int64_t B) {
  TetrisDesc d;
  memset(&d, 0, sizeof d);
  const int32_t ids[2] = {4, 3};
  if (tetris_host_desc_init(&d, 10, 20, ids, 2, nullptr) != 0) return 1;
  const int64_t words = tetris_host_board_words(&d, B), sw = tetris_host_status_words(B), nw = (B + 63) / 64;
  struct Env {
    std::vector<uint32_t> cols, status;
    std::vector<uint64_t> meta;
    std::vector<uint8_t> done, lines, nv, piece;
    std::vector<int32_t> act, rew;
    std::vector<float> obs;
  } e[2];
  int rc = 0;
  for (Env& x : e) {
    x.cols.assign(words, 0), x.status.assign(sw, 0), x.meta.assign(B, 0);
    x.done.assign(B, 0), x.lines.assign(B, 0), x.nv.assign(B, 0), x.piece.assign(B, 0);
    x.act.assign(B, 0), x.rew.assign(B, 0), x.obs.assign(B * 8, 0.f);
    rc |= tetris_host_reset(&d, x.cols.data(), x.meta.data(), nullptr, x.piece.data(), x.nv.data(), nullptr, nullptr, 0,
                            x.status.data(), 1, 7, 0, 0, B, nullptr);
  }
  std::vector<uint64_t> call((tetris_host_step_call_size() + 7) / 8), done_bits(nw, ~0ull);
  std::vector<uint32_t> snapshot(sw, 0);
  Env &a = e[0], &b = e[1];
  rc |= tetris_host_step_call_init(call.data(), &d, a.cols.data(), a.meta.data(), a.act.data(), nullptr, nullptr, 0, a.obs.data(),
                                   a.rew.data(), a.done.data(), a.lines.data(), a.nv.data(), a.piece.data(), a.status.data(),
                                   1, 7, 0, B);
  const uint64_t counter = 1;
  int bad = 0;
  for (uint64_t t = 0; t < 3; ++t) {
    if (t == 0) rc |= tetris_host_step_call_run(call.data(), nullptr, t, nullptr);
    if (t == 1) rc |= tetris_host_step_call_run_gather(call.data(), nullptr, t, done_bits.data(), snapshot.data(), nullptr);
    if (t == 2) rc |= tetris_host_step_call_run_counted(call.data(), nullptr, &counter, 1, nullptr);
    rc |= tetris_host_step(&d, b.cols.data(), b.meta.data(), nullptr, b.act.data(), nullptr, nullptr, 0, b.obs.data(),
                           b.rew.data(), b.done.data(), b.lines.data(), b.nv.data(), b.piece.data(), b.status.data(), 1, 7, t,
                           0, B, nullptr);
    bad += a.cols != b.cols || a.meta != b.meta || a.act != b.act || a.rew != b.rew || a.done != b.done ||
           a.status != b.status || a.obs != b.obs;
    if (t == 1) {
      std::vector<uint64_t> want(nw, 0);
      tetris_host_pack_done_bits(b.done.data(), reinterpret_cast<uint8_t*>(want.data()), B, nullptr);
      bad += want != done_bits || memcmp(snapshot.data(), b.status.data(), (size_t)nw * 16) != 0;
    }
  }
  printf("bound call, B = %lld: rc %d, %d mismatches\n", (long long)B, rc, bad);
  return rc | bad;
}

// calls the shared text must refuse before its backend is reached
static int refused() {
  TetrisDesc d, z;
  memset(&d, 0, sizeof d);
  memset(&z, 0, sizeof z);
  const int32_t ids[2] = {4, 3};
  if (tetris_host_desc_init(&d, 10, 20, ids, 2, nullptr) != 0) return 1;
  uint64_t word = 0;
  void* p = &word;
  uint8_t* b = reinterpret_cast<uint8_t*>(&word);
  std::vector<uint64_t> call((tetris_host_step_call_size() + 7) / 8, 0);
  int bad = 0;
  bad += tetris_host_step(&d, p, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, b, b, b, nullptr, nullptr, 0, 0, 0,
                          0, 16, nullptr) != TETRIS_E_NULL;
  bad += tetris_host_refresh(&z, p, &word, nullptr, 16, nullptr) != TETRIS_E_DESC;
  bad += tetris_host_reset(&d, p, &word, nullptr, nullptr, nullptr, b, nullptr, 4, nullptr, 1, 0, 0, 0, 16, nullptr) != TETRIS_E_STREAM;
  bad += tetris_host_afterstates(&d, p, &word, reinterpret_cast<float*>(p), b, nullptr, nullptr, 288, 6, 16, nullptr) != TETRIS_E_STRIDE;
  bad += tetris_host_rollouts(&d, p, &word, reinterpret_cast<double*>(p), 0, 2, 0, nullptr, nullptr, 0, 0, 0, 16, nullptr) != TETRIS_E_BATCH;
  bad += tetris_host_numpy_bag_stream(reinterpret_cast<uint32_t*>(p), 13, 8, b, 16, nullptr) != TETRIS_E_PIECES;
  bad += tetris_host_step_call_run(call.data(), nullptr, 0, nullptr) != TETRIS_E_DESC;
  bad += tetris_host_step_call_run_counted(call.data(), nullptr, nullptr, 0, nullptr) != TETRIS_E_NULL;
  printf("refused calls: %d wrong codes\n", bad + (word != 0));
  return bad + (word != 0);
}

int main() {
  const std::vector<int32_t> dflt = {4, 3}, std7 = {0, 7, 8, 1, 2, 5, 6};
  int rc = refused() | bound_call(256) | bound_call(100);
  for (int C : {10, 12, 11, 9, 5})
    for (int R : {20, 24, 40, 45}) {  // NCH = 2, 0 (u32, one plane per column), 4, 0 (u64, one plane per column)
      rc |= run(C, R, dflt, 256);
      rc |= run(C, R, std7, 256);
    }
  return rc;
}
