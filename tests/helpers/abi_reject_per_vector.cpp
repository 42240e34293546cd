// Driver of tests/test_per_vector_host.py — the rejected-argument paths of porl_per_fill_range and porl_per_sample_keyed on
// the HOST-ONLY sanitized build of csrc/porl_api.hip (-fsanitize=address,undefined), beside abi_reject_navsim.cpp.  Every
// call below must fail validation before it reaches a HIP call (or, for n == 0, return PORL_OK without one), so the program
// makes no launch and runs without a GPU.  Exit code 0 = every rejection was a clean error return with a message that names
// the argument, the buffers still hold their sentinels, and the sanitizers stayed silent (they abort the process otherwise).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../include/porl_hip.h"

static int g_checks = 0, g_bad = 0;
// a rejection must name what it refuses: `word` has to appear in the message
#define REJECT(word, expr)                                                                     \
  do {                                                                                         \
    ++g_checks;                                                                                \
    const long _r = (long)(expr);                                                              \
    const char* _m = porl_last_error();                                                        \
    if (_r == 0) { ++g_bad; std::fprintf(stderr, "accepted: %s\n", #expr); }                   \
    else if (_r != PORL_ERR_INVALID) { ++g_bad; std::fprintf(stderr, "code %ld: %s\n", _r, #expr); } \
    else if (!_m || !_m[0]) { ++g_bad; std::fprintf(stderr, "no message: %s\n", #expr); }      \
    else if (!std::strstr(_m, word)) { ++g_bad; std::fprintf(stderr, "message '%s' does not name '%s': %s\n", _m, word, #expr); } \
  } while (0)
#define ACCEPT(expr)                                                                           \
  do {                                                                                         \
    ++g_checks;                                                                                \
    if ((expr) != PORL_OK) { ++g_bad; std::fprintf(stderr, "refused: %s (%s)\n", #expr, porl_last_error()); } \
  } while (0)

int main() {
  if (porl_abi_version() != PORL_ABI_VERSION) return 2;
  // host memory standing in for device buffers: every call is refused before anything would touch them
  static double tree[15], scratch[4];
  static int64_t idx[4], slots[4];
  static float w[4], wmean[1];
  for (double& v : tree) v = 7.0;
  for (int i = 0; i < 4; ++i) { scratch[i] = 7.0; idx[i] = slots[i] = 7; w[i] = 7.f; }
  wmean[0] = 7.f;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
#define FILL(tree_, cap, first, n, td, eps, alpha) porl_per_fill_range(tree_, cap, first, n, td, eps, alpha, nullptr)
#define KEYED(tree_, cap, draw, batch, ne, idx_, slots_, w_, wm_, sc_) \
  porl_per_sample_keyed(tree_, cap, 5, draw, batch, ne, 0.4, idx_, slots_, w_, wm_, sc_, nullptr)
  // ---- porl_per_fill_range ------------------------------------------------------------------------------------------------
  REJECT("null tree", FILL(nullptr, 8, 0, 4, 1.0, 1e-5, 0.6));
  REJECT("capacity", FILL(tree, 0, 0, 0, 1.0, 1e-5, 0.6));
  REJECT("capacity", FILL(tree, -8, 0, 0, 1.0, 1e-5, 0.6));
  REJECT("capacity", FILL(tree, INT64_MAX, 0, 4, 1.0, 1e-5, 0.6));
  REJECT("n ", FILL(tree, 8, 0, -1, 1.0, 1e-5, 0.6));
  REJECT("n ", FILL(tree, 8, 0, 9, 1.0, 1e-5, 0.6));
  REJECT("n ", FILL(tree, 8, 0, INT64_MAX, 1.0, 1e-5, 0.6));
  REJECT("first_slot", FILL(tree, 8, -1, 4, 1.0, 1e-5, 0.6));
  REJECT("first_slot", FILL(tree, 8, 8, 4, 1.0, 1e-5, 0.6));
  REJECT("first_slot", FILL(tree, 8, INT64_MAX, 4, 1.0, 1e-5, 0.6));
  REJECT("first_slot", FILL(tree, 8, 8, 0, 1.0, 1e-5, 0.6));            // judged even when n == 0
  REJECT("td_error", FILL(tree, 8, 0, 4, nan, 1e-5, 0.6));
  REJECT("td_error", FILL(tree, 8, 0, 4, inf, 1e-5, 0.6));
  REJECT("td_error", FILL(tree, 8, 0, 4, -inf, 1e-5, 0.6));
  REJECT("eps", FILL(tree, 8, 0, 4, 1.0, nan, 0.6));
  REJECT("eps", FILL(tree, 8, 0, 4, 1.0, inf, 0.6));
  REJECT("alpha", FILL(tree, 8, 0, 4, 1.0, 1e-5, nan));
  REJECT("alpha", FILL(tree, 8, 0, 4, 1.0, 1e-5, -inf));
  ACCEPT(FILL(tree, 8, 0, 0, 1.0, 1e-5, 0.6));                          // n == 0: PORL_OK, no launch
  ACCEPT(FILL(tree, 8, 7, 0, 1.0, 1e-5, 0.6));
  ACCEPT(FILL(tree, 1, 0, 0, 1.0, 1e-5, 0.6));
  // ---- porl_per_sample_keyed ----------------------------------------------------------------------------------------------
  REJECT("null", KEYED(nullptr, 8, 0, 4, 8, idx, slots, w, wmean, scratch));
  REJECT("null", KEYED(tree, 8, 0, 4, 8, nullptr, slots, w, wmean, scratch));
  REJECT("null", KEYED(tree, 8, 0, 4, 8, idx, nullptr, w, wmean, scratch));
  REJECT("null", KEYED(tree, 8, 0, 4, 8, idx, slots, nullptr, wmean, scratch));
  REJECT("null", KEYED(tree, 8, 0, 4, 8, idx, slots, w, nullptr, scratch));
  REJECT("null", KEYED(tree, 8, 0, 4, 8, idx, slots, w, wmean, nullptr));
  REJECT("capacity", KEYED(tree, 0, 0, 4, 0, idx, slots, w, wmean, scratch));
  REJECT("batch", KEYED(tree, 8, 0, 0, 8, idx, slots, w, wmean, scratch));
  REJECT("batch", KEYED(tree, 8, 0, -4, 8, idx, slots, w, wmean, scratch));
  REJECT("n_entries", KEYED(tree, 8, 0, 4, 0, idx, slots, w, wmean, scratch));
  REJECT("n_entries", KEYED(tree, 8, 0, 4, 9, idx, slots, w, wmean, scratch));
  REJECT("draw", KEYED(tree, 8, -1, 4, 8, idx, slots, w, wmean, scratch));
  REJECT("draw", KEYED(tree, 8, int64_t(1) << 32, 4, 8, idx, slots, w, wmean, scratch));
  REJECT("draw", KEYED(tree, 8, INT64_MAX, 4, 8, idx, slots, w, wmean, scratch));
  // nothing was written
  ++g_checks;
  bool clean = wmean[0] == 7.f;
  for (double v : tree) clean = clean && v == 7.0;
  for (int i = 0; i < 4; ++i) clean = clean && scratch[i] == 7.0 && idx[i] == 7 && slots[i] == 7 && w[i] == 7.f;
  if (!clean) { ++g_bad; std::fprintf(stderr, "a rejected call wrote to its buffers\n"); }
  std::printf("abi_reject_per_vector: %d checks, %d unexpected\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
