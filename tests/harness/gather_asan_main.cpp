// Address / undefined-behaviour sanitizer driver for tetris_host_gather_envs (CPU only): the shared per-env body
// of the gather kernel (tet::gather_env) and the text of its C-ABI entry on heap buffers of EXACTLY their
// documented sizes, so that a write to a padding lane beyond B_dst -- in n_valid, piece, meta or past the last
// tile of cols -- is a heap overflow the sanitizer reports.  tests/test_gather_asan.py builds and runs it:
//   g++ -O0 -g1 -std=c++17 '-DTET_COLUMNS(X)=X(5) X(6) X(10) X(12)' -fsanitize=address,undefined -fno-sanitize-recover=undefined gather_asan_main.cpp -o gather_asan_main
// For every storage class (u32 / u64 words, packed / one plane per column) and two dst sizes with a partial last
// tile: a random index with repeats and -1 entries (the copy is exact, untouched envs keep every byte), then the
// same with out-of-range entries (untouched, counted in the slot of their dst wave).  The yardstick is the
// harness's own decode / afterstates of the SOURCE.  Any mismatch and anything the sanitizers report fails it.
#include "core_host.cpp"

#include <cstdio>
#include <memory>
#include <vector>

namespace {

template <typename T>
std::unique_ptr<T[]> exact(int64_t n) { return std::unique_ptr<T[]>(new T[n]()); }  // n elements, not one more

struct Batch {
  int64_t B = 0, words = 0, status_words = 0, cell_count = 0;
  std::unique_ptr<uint8_t[]> cols, n_valid, piece;  // cols: words * word_bytes bytes
  std::unique_ptr<uint64_t[]> meta;
  std::unique_ptr<uint32_t[]> status;
  std::unique_ptr<int8_t[]> cells;                  // decoded boards [B][R + 4][C]
  std::unique_ptr<uint8_t[]> after_n;               // n_valid as tetris_host_afterstates reports it
};

// B envs played `steps` random steps with auto-reset (boards, pieces and bags differ), then read out
int play(const TetrisDesc& d, Batch& e, int64_t B, uint64_t seed, int steps) {
  e.B = B;
  e.words = tetris_host_board_words(&d, B);
  e.status_words = tetris_host_status_words(B);
  e.cell_count = B * (d.num_rows + 4) * d.num_columns;
  e.cols = exact<uint8_t>(e.words * d.word_bytes);
  e.meta = exact<uint64_t>(B);
  e.n_valid = exact<uint8_t>(B);
  e.piece = exact<uint8_t>(B);
  e.status = exact<uint32_t>(e.status_words);
  int rc = tetris_host_reset(&d, e.cols.get(), e.meta.get(), nullptr, e.piece.get(), e.n_valid.get(), nullptr, nullptr, 0,
                             e.status.get(), 1, seed, 0, 0, B, nullptr);
  const int64_t n = (int64_t)steps * B;
  auto rew = exact<int32_t>(n);
  auto done = exact<uint8_t>(n), lines = exact<uint8_t>(n), nv = exact<uint8_t>(n), pc = exact<uint8_t>(n);
  rc |= tetris_host_step_many(&d, e.cols.get(), e.meta.get(), steps, 0, nullptr, nullptr, nullptr, rew.get(), done.get(),
                              lines.get(), nv.get(), pc.get(), e.status.get(), 1, seed, 0, 0, B, nullptr);
  memcpy(e.n_valid.get(), nv.get() + (n - B), B);
  memcpy(e.piece.get(), pc.get() + (n - B), B);
  return rc;
}

int read_out(const TetrisDesc& d, Batch& e) {
  e.cells = exact<int8_t>(e.cell_count);
  e.after_n = exact<uint8_t>(e.B);
  auto feats = exact<float>(e.B * d.a_max * 8);
  return tetris_host_decode(&d, e.cols.get(), e.cells.get(), nullptr, e.B, nullptr) |
         tetris_host_afterstates(&d, e.cols.get(), e.meta.get(), feats.get(), e.after_n.get(), nullptr, nullptr, d.a_max * 8, 8,
                                 e.B, nullptr);
}

uint32_t g_rng = 12345;
uint32_t rnd() { return (g_rng = g_rng * 1664525u + 1013904223u) >> 8; }

// one gather of src into a fresh dst under `index`; returns the number of mismatches
int64_t check(const TetrisDesc& d, const Batch& src, int64_t B_dst, const std::vector<int32_t>& index) {
  Batch dst;
  if (play(d, dst, B_dst, 11, 17) || read_out(d, dst)) return 1000;
  const int np = tetris_host_n_planes(&d), wb = d.word_bytes;
  const int64_t cols_bytes = dst.words * wb, env_cells = (d.num_rows + 4) * d.num_columns;
  std::vector<uint8_t> cols0(dst.cols.get(), dst.cols.get() + cols_bytes), nv0(dst.n_valid.get(), dst.n_valid.get() + B_dst),
      pc0(dst.piece.get(), dst.piece.get() + B_dst);
  std::vector<uint64_t> meta0(dst.meta.get(), dst.meta.get() + B_dst);
  std::vector<uint32_t> status0(dst.status.get(), dst.status.get() + dst.status_words);
  std::vector<int8_t> cells0(dst.cells.get(), dst.cells.get() + dst.cell_count);
  auto idx = exact<int32_t>(B_dst);
  for (int64_t j = 0; j < B_dst; ++j) idx[j] = index[j];

  if (tetris_host_gather_envs(&d, src.cols.get(), src.meta.get(), src.B, dst.cols.get(), dst.meta.get(), dst.n_valid.get(),
                              dst.piece.get(), idx.get(), dst.status.get(), B_dst, nullptr) != TETRIS_OK)
    return 1000;

  int64_t bad = 0;
  if (read_out(d, dst)) return 1000;
  std::vector<uint32_t> want_status = status0;
  auto word = [&](const uint8_t* cols, int64_t i, int q) { return cols + ((((i >> 6) * np + q) << 6) + (i & 63)) * wb; };
  for (int64_t j = 0; j < B_dst; ++j) {
    const int32_t s = index[j];
    if (s >= 0 && s < src.B) {  // copied: the source's read-outs, every stored word, all 64 bits of meta
      bad += memcmp(dst.cells.get() + j * env_cells, src.cells.get() + s * env_cells, env_cells) != 0;
      bad += dst.meta[j] != src.meta[s];
      bad += dst.n_valid[j] != src.after_n[s] || dst.n_valid[j] != src.n_valid[s] || dst.after_n[j] != src.after_n[s];
      bad += dst.piece[j] != src.piece[s];
      for (int q = 0; q < np; ++q) bad += memcmp(word(dst.cols.get(), j, q), word(src.cols.get(), s, q), wb) != 0;
    } else {                    // kept: every byte as before
      bad += memcmp(dst.cells.get() + j * env_cells, cells0.data() + j * env_cells, env_cells) != 0;
      bad += dst.meta[j] != meta0[j] || dst.n_valid[j] != nv0[j] || dst.piece[j] != pc0[j];
      for (int q = 0; q < np; ++q) bad += memcmp(word(dst.cols.get(), j, q), word(cols0.data(), j, q), wb) != 0;
      if (s != -1) want_status[(j >> 6) * 4 + TETRIS_STATUS_INVALID] += 1;
    }
  }
  for (int64_t j = B_dst; j < (B_dst + 63) / 64 * 64; ++j)  // the padding lanes of the last tile
    for (int q = 0; q < np; ++q) bad += memcmp(word(dst.cols.get(), j, q), word(cols0.data(), j, q), wb) != 0;
  bad += memcmp(want_status.data(), dst.status.get(), dst.status_words * 4) != 0;
  return bad;
}

int64_t run(int C, int R, const std::vector<int32_t>& ids) {
  TetrisDesc d;
  memset(&d, 0, sizeof d);
  if (tetris_host_desc_init(&d, C, R, ids.data(), (int32_t)ids.size(), nullptr) != 0) return 1000;
  const int64_t B_src = 200;
  Batch src;
  if (play(d, src, B_src, 3, 30) || read_out(d, src)) return 1000;
  int64_t bad = 0;
  for (int64_t B_dst : {130, 321}) {
    std::vector<int32_t> index(B_dst);
    for (int64_t j = 0; j < B_dst; ++j) index[j] = rnd() % 4 == 0 ? -1 : (int32_t)(rnd() % B_src);  // repeats, a quarter kept
    index[0] = 0, index[1] = (int32_t)B_src - 1, index[2] = -1, index[B_dst - 2] = -1, index[B_dst - 1] = (int32_t)B_src - 1;
    bad += check(d, src, B_dst, index);                                                          // case 1
    index[5] = (int32_t)B_src, index[70] = -2, index[B_dst - 1] = 0x7FFFFFFF, index[B_dst - 3] = INT32_MIN;
    bad += check(d, src, B_dst, index);                                                          // case 3
  }
  printf("%2d x %2d, %zu pieces, %d planes of %d bytes: %lld mismatches\n", C, R, ids.size(), tetris_host_n_planes(&d),
         d.word_bytes, (long long)bad);
  return bad;
}

}  // namespace

int main() {
  const std::vector<int32_t> dflt = {4, 3}, std7 = {0, 7, 8, 1, 2, 5, 6};
  int64_t bad = 0;
  bad += run(10, 20, dflt);  // u32, packed
  bad += run(6, 26, dflt);   // u32, one plane per column
  bad += run(10, 40, std7);  // u64, packed
  bad += run(5, 50, dflt);   // u64, one plane per column
  bad += run(12, 20, dflt);  // nine planes
  printf("mismatches: %lld\n", (long long)bad);
  return bad != 0;
}
