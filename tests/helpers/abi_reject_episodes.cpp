// Driver of tests/test_episodes_host.py — the rejected-argument paths of the episode entry points (porl_episode_workspace,
// porl_episode_count, porl_episode_fill, porl_episode_returns, porl_hindsight_pairs, porl_gather_pairs) on the HOST-ONLY
// sanitized build of csrc/porl_api.hip (-fsanitize=address,undefined), beside abi_reject.cpp and abi_reject_rows.cpp.
// Every call below must fail validation before it reaches a HIP call, so the program makes no launch and runs without
// a GPU.  Exit code 0 = every rejection was a clean error return with a message that names the argument and the
// sanitizers stayed silent (they abort the process otherwise).
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
  const int64_t BIG = (int64_t(1) << 40) + 1;
  float f[64] = {0};
  double d[64] = {0};
  int64_t i[64] = {0};
  // ---- porl_episode_workspace (pure host) -----------------------------------------------------------------------------
  int32_t T = 0, P = 0;
  EXPECT(porl_episode_workspace(1, &T, &P) == 7 && T >= 64 && P >= 1);
  EXPECT(porl_episode_workspace((int64_t)T, nullptr, nullptr) == 7);
  EXPECT(porl_episode_workspace((int64_t)T + 1, nullptr, nullptr) == 12);
  EXPECT(porl_episode_workspace(int64_t(1) << 40, nullptr, nullptr) == 2 + 5 * ((int64_t(1) << 40) / T));
  REJECT("n_rows", porl_episode_workspace(0, nullptr, nullptr));
  REJECT("n_rows", porl_episode_workspace(-3, &T, &P));
  REJECT("n_rows", porl_episode_workspace(BIG, nullptr, nullptr));
  // ---- porl_episode_count ---------------------------------------------------------------------------------------------
  REJECT("null flags", porl_episode_count(nullptr, 1, 8, 0, i, nullptr));
  REJECT("null workspace", porl_episode_count(f, 1, 8, 0, nullptr, nullptr));
  REJECT("n_rows", porl_episode_count(f, 1, 0, 0, i, nullptr));
  REJECT("n_rows", porl_episode_count(f, 1, -1, 0, i, nullptr));
  REJECT("n_rows", porl_episode_count(f, 1, BIG, 0, i, nullptr));
  REJECT("stride", porl_episode_count(f, 0, 8, 0, i, nullptr));
  REJECT("stride", porl_episode_count(f, -4, 8, 0, i, nullptr));
  REJECT("stride", porl_episode_count(f, INT64_MAX, 8, 0, i, nullptr));
  REJECT("cap", porl_episode_count(f, 1, 8, -1, i, nullptr));
  REJECT("cap", porl_episode_count(f, 1, 8, INT64_MIN, i, nullptr));
  // ---- porl_episode_fill ------------------------------------------------------------------------------------------------
  REJECT("null flags", porl_episode_fill(nullptr, 1, 8, 0, i, 2, i, i, nullptr));
  REJECT("null workspace", porl_episode_fill(f, 1, 8, 0, nullptr, 2, i, i, nullptr));
  REJECT("null starts", porl_episode_fill(f, 1, 8, 0, i, 2, nullptr, i, nullptr));
  REJECT("null ends", porl_episode_fill(f, 1, 8, 0, i, 2, i, nullptr, nullptr));
  REJECT("n_rows", porl_episode_fill(f, 1, 0, 0, i, 2, i, i, nullptr));
  REJECT("n_rows", porl_episode_fill(f, 1, BIG, 0, i, 2, i, i, nullptr));
  REJECT("stride", porl_episode_fill(f, 0, 8, 0, i, 2, i, i, nullptr));
  REJECT("cap", porl_episode_fill(f, 1, 8, -7, i, 2, i, i, nullptr));
  REJECT("n_episodes", porl_episode_fill(f, 1, 8, 0, i, 0, i, i, nullptr));
  REJECT("n_episodes", porl_episode_fill(f, 1, 8, 0, i, -1, i, i, nullptr));
  REJECT("n_episodes", porl_episode_fill(f, 1, 8, 0, i, 9, i, i, nullptr));          // more episodes than rows
  // ---- porl_episode_returns ---------------------------------------------------------------------------------------------
  REJECT("null rewards", porl_episode_returns(nullptr, 1, 8, i, i, 2, d, i, d, nullptr));
  REJECT("null starts", porl_episode_returns(f, 1, 8, nullptr, i, 2, d, i, d, nullptr));
  REJECT("null ends", porl_episode_returns(f, 1, 8, i, nullptr, 2, d, i, d, nullptr));
  REJECT("null returns", porl_episode_returns(f, 1, 8, i, i, 2, nullptr, i, d, nullptr));
  REJECT("null range_ws", porl_episode_returns(f, 1, 8, i, i, 2, d, nullptr, d, nullptr));
  REJECT("n_rows", porl_episode_returns(f, 1, 0, i, i, 2, d, i, d, nullptr));
  REJECT("n_rows", porl_episode_returns(f, 1, BIG, i, i, 2, d, i, d, nullptr));
  REJECT("stride", porl_episode_returns(f, 0, 8, i, i, 2, d, i, d, nullptr));
  REJECT("stride", porl_episode_returns(f, -1, 8, i, i, 2, d, nullptr, nullptr, nullptr));
  REJECT("n_episodes", porl_episode_returns(f, 1, 8, i, i, 0, d, i, d, nullptr));
  REJECT("n_episodes", porl_episode_returns(f, 1, 8, i, i, 9, d, i, d, nullptr));
  // ---- porl_hindsight_pairs -----------------------------------------------------------------------------------------------
  REJECT("null starts", porl_hindsight_pairs(nullptr, i, 3, 8, 0, 0, nullptr, nullptr, nullptr, i, i, nullptr, nullptr, nullptr, nullptr));
  REJECT("null lengths", porl_hindsight_pairs(i, nullptr, 3, 8, 0, 0, nullptr, nullptr, nullptr, i, i, nullptr, nullptr, nullptr, nullptr));
  REJECT("null start", porl_hindsight_pairs(i, i, 3, 8, 0, 0, nullptr, nullptr, nullptr, nullptr, i, nullptr, nullptr, nullptr, nullptr));
  REJECT("null goal", porl_hindsight_pairs(i, i, 3, 8, 0, 0, nullptr, nullptr, nullptr, i, nullptr, nullptr, nullptr, nullptr, nullptr));
  REJECT("n_episodes", porl_hindsight_pairs(i, i, 0, 8, 0, 0, nullptr, nullptr, nullptr, i, i, nullptr, nullptr, nullptr, nullptr));
  REJECT("n_episodes", porl_hindsight_pairs(i, i, -2, 8, 0, 0, nullptr, nullptr, nullptr, i, i, nullptr, nullptr, nullptr, nullptr));
  REJECT("n_episodes", porl_hindsight_pairs(i, i, BIG, 8, 0, 0, nullptr, nullptr, nullptr, i, i, nullptr, nullptr, nullptr, nullptr));
  REJECT("batch", porl_hindsight_pairs(i, i, 3, 0, 0, 0, nullptr, nullptr, nullptr, i, i, nullptr, nullptr, nullptr, nullptr));
  REJECT("batch", porl_hindsight_pairs(i, i, 3, -8, 0, 0, nullptr, nullptr, nullptr, i, i, nullptr, nullptr, nullptr, nullptr));
  REJECT("null traj", porl_hindsight_pairs(i, i, 3, 8, 0, 0, nullptr, d, d, i, i, nullptr, nullptr, nullptr, nullptr));
  REJECT("null u1", porl_hindsight_pairs(i, i, 3, 8, 0, 0, i, nullptr, d, i, i, nullptr, nullptr, nullptr, nullptr));
  REJECT("null u2", porl_hindsight_pairs(i, i, 3, 8, 0, 0, i, d, nullptr, i, i, nullptr, nullptr, nullptr, nullptr));
  // ---- porl_gather_pairs ------------------------------------------------------------------------------------------------
  // S = 5, A = 1: rows of 13 floats
  REJECT("null rows", porl_gather_pairs(nullptr, 13, 4, i, i, 2, 5, 1, f, 13, nullptr));
  REJECT("null start", porl_gather_pairs(f, 13, 4, nullptr, i, 2, 5, 1, f, 13, nullptr));
  REJECT("null goal", porl_gather_pairs(f, 13, 4, i, nullptr, 2, 5, 1, f, 13, nullptr));
  REJECT("null out", porl_gather_pairs(f, 13, 4, i, i, 2, 5, 1, nullptr, 13, nullptr));
  REJECT("n_rows", porl_gather_pairs(f, 13, 0, i, i, 2, 5, 1, f, 13, nullptr));
  REJECT("n_rows", porl_gather_pairs(f, 13, BIG, i, i, 2, 5, 1, f, 13, nullptr));
  REJECT("batch", porl_gather_pairs(f, 13, 4, i, i, 0, 5, 1, f, 13, nullptr));
  REJECT("batch", porl_gather_pairs(f, 13, 4, i, i, -1, 5, 1, f, 13, nullptr));
  REJECT("obs_dim", porl_gather_pairs(f, 13, 4, i, i, 2, 0, 1, f, 13, nullptr));
  REJECT("obs_dim", porl_gather_pairs(f, 13, 4, i, i, 2, INT32_MAX, 1, f, 13, nullptr));
  REJECT("act_dim", porl_gather_pairs(f, 13, 4, i, i, 2, 5, -1, f, 13, nullptr));
  REJECT("act_dim", porl_gather_pairs(f, 13, 4, i, i, 2, 5, INT32_MAX, f, 13, nullptr));
  REJECT("row_stride", porl_gather_pairs(f, 12, 4, i, i, 2, 5, 1, f, 13, nullptr));
  REJECT("row_stride", porl_gather_pairs(f, 0, 4, i, i, 2, 5, 1, f, 13, nullptr));
  REJECT("row_stride", porl_gather_pairs(f, INT64_MAX, 4, i, i, 2, 5, 1, f, 13, nullptr));
  REJECT("out_stride", porl_gather_pairs(f, 13, 4, i, i, 2, 5, 1, f, 12, nullptr));
  REJECT("out_stride", porl_gather_pairs(f, 13, 4, i, i, 2, 5, 1, f, -13, nullptr));
  std::printf("abi_reject_episodes: %d checks, %d unexpected\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
