// Address / undefined-behaviour sanitizer driver for the lane-test harness (CPU only; not part of the test suite):
//   make -C tests/harness lane_asan
// builds it, writes the clean golden boards of set (iii) to golden_clean.u32 (ten little-endian uint32 column
// words per board, from golden_clean_cols() of tests/test_step_lane_equivalence.py) and runs it on them.
// It runs 20,000 window boards on ten columns and 12,000 on eight, both piece sets, and the boards of the file
// through lane_boards and the yardstick's own entries.  Any mismatch, a missing file, and anything the
// sanitizers report, fails it.
#include "lane_equivalence.cpp"

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
  const std::vector<int32_t> dflt = {4, 3}, cat9 = {0, 1, 2, 3, 4, 5, 6, 7, 8};
  int64_t bad = 0;
  for (int C : {10, 8})
    for (const auto& ids : {dflt, cat9}) {
      int64_t rescued[16] = {0}, checked = 0, feat_bad = 0;
      bad += lane_vm_window(C, 20, (int)ids.size(), ids.data(), 0x7E7215 + 20, 4194, rescued, &checked, &feat_bad) + feat_bad;
      printf("window C=%d, %zu pieces: %lld masks compared\n", C, ids.size(), (long long)checked);
    }
  {
    std::vector<uint32_t> cols;
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    for (uint32_t w; fread(&w, sizeof(w), 1, f) == 1;) cols.push_back(w);
    fclose(f);
    const int64_t n = (int64_t)cols.size() / 10;
    int64_t out[6] = {0};
    lane_boards(20, (int)cat9.size(), cat9.data(), cols.data(), n, out);
    std::vector<uint64_t> masks(n);
    std::vector<int32_t> feats(6 * n);
    for (int pid = 0; pid < 9; ++pid) lane_yardstick_masks(20, pid, cols.data(), n, masks.data());
    lane_yardstick_features(20, cols.data(), n, feats.data());
    printf("%lld boards from %s: %lld masks compared, %lld dirty\n", (long long)n, argv[1], (long long)out[3], (long long)out[2]);
    bad += out[0] + out[1] + out[2];
  }
  printf("mismatches: %lld\n", (long long)bad);
  return bad != 0;
}
