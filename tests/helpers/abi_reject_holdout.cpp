// Driver of tests/test_holdout_host.py — the rejected-argument paths of the partition entry points
// (porl_partition_workspace, porl_partition_mask, porl_partition_rows) on the HOST-ONLY sanitized build of
// csrc/porl_api.hip (-fsanitize=address,undefined), beside abi_reject_episodes.cpp.  Every call below must fail
// validation before it reaches a HIP call, so the program makes no launch and runs without a GPU.  Exit code 0 = every
// rejection was a clean error return with a message that names the argument and the sanitizers stayed silent (they
// abort the process otherwise).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/porl_hip.h"

static int g_checks = 0, g_bad = 0;
// a rejection must name what it refuses: `word` has to appear in the message
#define REJECT(word, expr)                                                                     \
  do {                                                                                         \
    ++g_checks;                                                                                \
    const long _r = (long)(expr);                                                              \
    const char* _m = porl_last_error();                                                        \
    if (_r != -1) { ++g_bad; std::fprintf(stderr, "returned %ld: %s\n", _r, #expr); }          \
    else if (!_m || !_m[0]) { ++g_bad; std::fprintf(stderr, "no message: %s\n", #expr); }      \
    else if (!std::strstr(_m, word)) { ++g_bad; std::fprintf(stderr, "message '%s' does not name '%s': %s\n", _m, word, #expr); } \
  } while (0)
#define EXPECT(cond)                                                                           \
  do {                                                                                         \
    ++g_checks;                                                                                \
    if (!(cond)) { ++g_bad; std::fprintf(stderr, "failed: %s\n", #cond); }                     \
  } while (0)

int main() {
  if (porl_abi_version() != PORL_ABI_VERSION) return 2;
  const int64_t BIG = (int64_t(1) << 36) + 1;
  alignas(16) float f[256] = {0};
  alignas(16) float o[256] = {0};
  uint8_t m[64] = {0};
  int64_t w[64] = {0}, ix[64] = {0};
  const porl_partition_box box = {0, 1, 5.f, 10.f, 2.f, 7.f};
  // ---- porl_partition_workspace (pure host) ---------------------------------------------------------------------------
  int32_t T = 0, P = 0;
  EXPECT(porl_partition_workspace(1, &T, &P) == 4 && T >= 64 && P >= 1);
  EXPECT(porl_partition_workspace((int64_t)T, nullptr, nullptr) == 4);
  EXPECT(porl_partition_workspace((int64_t)T + 1, nullptr, nullptr) == 6);
  EXPECT(porl_partition_workspace((int64_t)T * P + 1, nullptr, nullptr) == 2 + 2 * ((int64_t)P + 1));
  REJECT("n_rows", porl_partition_workspace(0, nullptr, nullptr));
  REJECT("n_rows", porl_partition_workspace(-3, &T, &P));
  REJECT("n_rows", porl_partition_workspace(BIG, nullptr, nullptr));
  // ---- porl_partition_mask: 8 rows of 4 floats ----------------------------------------------------------------------------
  REJECT("null rows", porl_partition_mask(nullptr, 16, 8, 16, &box, m, nullptr));
  REJECT("null box", porl_partition_mask(f, 16, 8, 16, nullptr, m, nullptr));
  REJECT("null mask", porl_partition_mask(f, 16, 8, 16, &box, nullptr, nullptr));
  REJECT("n_rows", porl_partition_mask(f, 16, 0, 16, &box, m, nullptr));
  REJECT("n_rows", porl_partition_mask(f, 16, -1, 16, &box, m, nullptr));
  REJECT("n_rows", porl_partition_mask(f, 16, BIG, 16, &box, m, nullptr));
  REJECT("row_bytes", porl_partition_mask(f, 16, 8, 0, &box, m, nullptr));
  REJECT("row_bytes", porl_partition_mask(f, 16, 8, 6, &box, m, nullptr));
  REJECT("row_bytes", porl_partition_mask(f, 16, 8, -16, &box, m, nullptr));
  REJECT("stride_bytes", porl_partition_mask(f, 12, 8, 16, &box, m, nullptr));
  REJECT("stride_bytes", porl_partition_mask(f, 18, 8, 16, &box, m, nullptr));
  REJECT("stride_bytes", porl_partition_mask(f, -16, 8, 16, &box, m, nullptr));
  REJECT("stride_bytes", porl_partition_mask(f, INT64_MAX, 8, 16, &box, m, nullptr));
  REJECT("aligned", porl_partition_mask(reinterpret_cast<const char*>(f) + 2, 16, 8, 16, &box, m, nullptr));
  {
    porl_partition_box b = box;
    b.cx = 4;
    REJECT("cx", porl_partition_mask(f, 16, 8, 16, &b, m, nullptr));
    b.cx = -1;
    REJECT("cx", porl_partition_mask(f, 16, 8, 16, &b, m, nullptr));
    b = box;
    b.cy = 4;
    REJECT("cy", porl_partition_mask(f, 16, 8, 16, &b, m, nullptr));
    b.cy = INT32_MIN;
    REJECT("cy", porl_partition_rows(f, 16, 8, 16, nullptr, &b, o, ix, w, nullptr));
    b = box;
    b.cx = INT32_MAX;
    REJECT("cx", porl_partition_rows(f, 16, 8, 16, nullptr, &b, o, ix, w, nullptr));
  }
  // ---- porl_partition_rows ----------------------------------------------------------------------------------------------
  REJECT("null rows", porl_partition_rows(nullptr, 16, 8, 16, m, nullptr, o, ix, w, nullptr));
  REJECT("null out", porl_partition_rows(f, 16, 8, 16, m, nullptr, nullptr, ix, w, nullptr));
  REJECT("null workspace", porl_partition_rows(f, 16, 8, 16, m, nullptr, o, ix, nullptr, nullptr));
  REJECT("both", porl_partition_rows(f, 16, 8, 16, m, &box, o, ix, w, nullptr));
  REJECT("neither", porl_partition_rows(f, 16, 8, 16, nullptr, nullptr, o, ix, w, nullptr));
  REJECT("n_rows", porl_partition_rows(f, 16, 0, 16, m, nullptr, o, nullptr, w, nullptr));
  REJECT("n_rows", porl_partition_rows(f, 16, -8, 16, m, nullptr, o, nullptr, w, nullptr));
  REJECT("n_rows", porl_partition_rows(f, 16, BIG, 16, nullptr, &box, o, nullptr, w, nullptr));
  REJECT("row_bytes", porl_partition_rows(f, 16, 8, 0, m, nullptr, o, nullptr, w, nullptr));
  REJECT("row_bytes", porl_partition_rows(f, 16, 8, 2, m, nullptr, o, nullptr, w, nullptr));
  REJECT("row_bytes", porl_partition_rows(f, 16, 8, 15, nullptr, &box, o, nullptr, w, nullptr));
  REJECT("row_bytes", porl_partition_rows(f, 16, 8, -4, m, nullptr, o, nullptr, w, nullptr));
  REJECT("row_bytes", porl_partition_rows(f, INT64_MAX, 8, INT64_MAX - 3, m, nullptr, o, nullptr, w, nullptr));
  REJECT("stride_bytes", porl_partition_rows(f, 8, 8, 16, m, nullptr, o, nullptr, w, nullptr));
  REJECT("stride_bytes", porl_partition_rows(f, 0, 8, 16, m, nullptr, o, nullptr, w, nullptr));
  REJECT("stride_bytes", porl_partition_rows(f, 17, 8, 16, m, nullptr, o, nullptr, w, nullptr));
  REJECT("stride_bytes", porl_partition_rows(f, INT64_MIN, 8, 16, m, nullptr, o, nullptr, w, nullptr));
  REJECT("aligned", porl_partition_rows(reinterpret_cast<const char*>(f) + 1, 16, 8, 16, m, nullptr, o, nullptr, w, nullptr));
  REJECT("aligned", porl_partition_rows(f, 16, 8, 16, m, nullptr, reinterpret_cast<char*>(o) + 2, nullptr, w, nullptr));
  std::printf("abi_reject_holdout: %d checks, %d unexpected\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
