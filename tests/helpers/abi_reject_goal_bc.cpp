// Driver of tests/test_goal_bc_host.py — the rejected-argument paths of the goal-conditioned behaviour-cloning entry
// points (porl_iql_load_batch_cat, porl_iql_load_batch_pairs, porl_iql_bc_forward, porl_iql_bc_step) on the HOST-ONLY
// sanitized build of csrc/porl_api.hip (-fsanitize=address,undefined), beside abi_reject_rows.cpp.  Every call below must
// fail validation before it reaches a HIP call, so the program makes no launch and runs without a GPU.  Exit code 0 =
// every rejection was a clean error return with a message that names the argument and the sanitizers stayed silent
// (they abort the process otherwise).
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
    if (_r == 0) { ++g_bad; std::fprintf(stderr, "accepted: %s\n", #expr); }                   \
    else if (!_m || !_m[0]) { ++g_bad; std::fprintf(stderr, "no message: %s\n", #expr); }      \
    else if (!std::strstr(_m, word)) { ++g_bad; std::fprintf(stderr, "message '%s' does not name '%s': %s\n", _m, word, #expr); } \
  } while (0)
#define ACCEPT(expr)                                                                           \
  do {                                                                                         \
    ++g_checks;                                                                                \
    const long _r = (long)(expr);                                                              \
    if (_r != 0) { ++g_bad; std::fprintf(stderr, "rejected (%ld, %s): %s\n", _r, porl_last_error(), #expr); } \
  } while (0)

static float* mk(int64_t n) { return static_cast<float*>(std::aligned_alloc(64, ((size_t)(n > 0 ? n : 1) * 4 + 63) / 64 * 64)); }

int main() {
  if (porl_abi_version() != PORL_ABI_VERSION) return 2;
  float x[64] = {0};
  int64_t ix[8] = {0}, tab[8] = {0};
  porl_iql_hyper hp{};
  hp.inv_batch = 1.f; hp.policy_step = 1; hp.policy_lr = 1e-4; hp.adam_beta1 = 0.9; hp.adam_beta2 = 0.999; hp.adam_eps = 1e-8;
  // pi(a | s, g) on 60-wide states with 60-wide goals and 2 actions: obs_dim 120, rows of 2*60 + 2 + 2 = 124 floats
  porl_iql* h = nullptr;
  porl_iql_cfg c{120, 2, 64, 2, 0, 0, 1, 128};
  ACCEPT(porl_iql_create(&c, &h));
  // ---- before bind --------------------------------------------------------------------------------------------------------
  REJECT("null engine", porl_iql_load_batch_cat(nullptr, 8, x, 60, x, 60, 60, x, 2, nullptr));
  REJECT("bind", porl_iql_load_batch_cat(h, 8, x, 60, x, 60, 60, x, 2, nullptr));
  REJECT("null engine", porl_iql_load_batch_pairs(nullptr, 8, x, 124, 100, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr));
  REJECT("bind", porl_iql_load_batch_pairs(h, 8, x, 124, 100, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr));
  REJECT("null engine", porl_iql_bc_step(nullptr, &hp, nullptr));
  REJECT("null engine", porl_iql_bc_forward(nullptr, &hp, nullptr));
  REJECT("bind", porl_iql_bc_step(h, &hp, nullptr));
  REJECT("bind", porl_iql_bc_forward(h, &hp, nullptr));
  const int64_t nv = porl_iql_group_floats(h, 0), np_ = porl_iql_group_floats(h, 1), nw = porl_iql_workspace_floats(h);
  // host memory standing in for device buffers: bind only records the pointers (they are never dereferenced on the host)
  float* P[11] = {mk(nv), mk(nv), mk(np_), mk(nv), mk(np_), mk(nv), mk(nv), mk(np_), mk(np_), mk(nw), mk(8)};
  porl_iql_buffers bufs{P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7], P[8], P[9], P[10]};
  ACCEPT(porl_iql_bind(h, &bufs));
  // ---- the step needs a batch -------------------------------------------------------------------------------------------
  REJECT("no minibatch loaded", porl_iql_bc_step(h, &hp, nullptr));
  REJECT("no minibatch loaded", porl_iql_bc_forward(h, &hp, nullptr));
  // ---- porl_iql_load_batch_cat --------------------------------------------------------------------------------------------
  REJECT("batch", porl_iql_load_batch_cat(h, 0, x, 60, x, 60, 60, x, 2, nullptr));
  REJECT("batch", porl_iql_load_batch_cat(h, 129, x, 60, x, 60, 60, x, 2, nullptr));
  REJECT("batch", porl_iql_load_batch_cat(h, -4, x, 60, x, 60, 60, x, 2, nullptr));
  REJECT("null obs", porl_iql_load_batch_cat(h, 8, nullptr, 60, x, 60, 60, x, 2, nullptr));
  REJECT("null goals", porl_iql_load_batch_cat(h, 8, x, 60, nullptr, 60, 60, x, 2, nullptr));
  REJECT("null actions", porl_iql_load_batch_cat(h, 8, x, 60, x, 60, 60, nullptr, 2, nullptr));
  REJECT("goal_dim", porl_iql_load_batch_cat(h, 8, x, 60, x, 60, 0, x, 2, nullptr));
  REJECT("goal_dim", porl_iql_load_batch_cat(h, 8, x, 60, x, 60, -1, x, 2, nullptr));
  REJECT("goal_dim", porl_iql_load_batch_cat(h, 8, x, 60, x, 60, 120, x, 2, nullptr));        // leaves no observation column
  REJECT("goal_dim", porl_iql_load_batch_cat(h, 8, x, 60, x, 60, INT32_MAX, x, 2, nullptr));
  REJECT("obs_rs", porl_iql_load_batch_cat(h, 8, x, 59, x, 60, 60, x, 2, nullptr));
  REJECT("obs_rs", porl_iql_load_batch_cat(h, 8, x, 60, x, 2, 2, x, 2, nullptr));             // goal_dim 2: 118 observation columns
  REJECT("goals_rs", porl_iql_load_batch_cat(h, 8, x, 60, x, 59, 60, x, 2, nullptr));
  REJECT("goals_rs", porl_iql_load_batch_cat(h, 8, x, 60, x, -60, 60, x, 2, nullptr));
  REJECT("act_rs", porl_iql_load_batch_cat(h, 8, x, 60, x, 60, 60, x, 1, nullptr));
  REJECT("act_rs", porl_iql_load_batch_cat(h, 8, x, 60, x, 60, 60, x, 0, nullptr));
  // ---- porl_iql_load_batch_pairs ----------------------------------------------------------------------------------------
#define PAIRS(batch, rows, rs, n, S, A, gc, G, st, go, es, el, E) \
  porl_iql_load_batch_pairs(h, batch, rows, rs, n, S, A, gc, G, st, go, es, el, E, 1, 2, nullptr, nullptr, nullptr)
  REJECT("batch", PAIRS(0, x, 124, 100, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("batch", PAIRS(129, x, 124, 100, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("null rows", PAIRS(8, nullptr, 124, 100, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("n_rows", PAIRS(8, x, 124, 0, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("n_rows", PAIRS(8, x, 124, -7, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("n_rows", PAIRS(8, x, 124, (int64_t(1) << 40) + 1, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("n_rows", PAIRS(8, x, 124, 7, 60, 2, 61, 60, nullptr, nullptr, nullptr, nullptr, 0));      // 8 distinct rows of 7
  REJECT("state_dim", PAIRS(8, x, 124, 100, 0, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("act_dim", PAIRS(8, x, 124, 100, 60, 0, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("goal_dim", PAIRS(8, x, 124, 100, 60, 2, 61, 0, ix, ix, nullptr, nullptr, 0));
  REJECT("row_stride", PAIRS(8, x, 123, 100, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("row_stride", PAIRS(8, x, 0, 100, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("row_stride", PAIRS(8, x, -124, 100, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("row_stride", PAIRS(8, x, INT64_MAX, 100, 60, 2, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("goal_col", PAIRS(8, x, 124, 100, 60, 2, -1, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("goal_col", PAIRS(8, x, 124, 100, 60, 2, 63, 60, ix, ix, nullptr, nullptr, 0));            // 63 + 60 > 122
  REJECT("goal_col", PAIRS(8, x, 124, 100, 60, 2, INT32_MAX, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("obs_dim", PAIRS(8, x, 124, 100, 60, 2, 0, 2, ix, ix, nullptr, nullptr, 0));               // 60 + 2 != 120
  REJECT("obs_dim", PAIRS(8, x, 200, 100, 59, 2, 0, 59, ix, ix, nullptr, nullptr, 0));
  REJECT("pol_out_dim", PAIRS(8, x, 125, 100, 60, 3, 61, 60, ix, ix, nullptr, nullptr, 0));
  REJECT("null start", PAIRS(8, x, 124, 100, 60, 2, 0, 60, nullptr, ix, nullptr, nullptr, 0));      // a goal without a start
  REJECT("ep_lengths", PAIRS(8, x, 124, 100, 60, 2, 0, 60, nullptr, nullptr, tab, nullptr, 4));
  REJECT("ep_starts", PAIRS(8, x, 124, 100, 60, 2, 0, 60, nullptr, nullptr, nullptr, tab, 4));
  REJECT("n_episodes", PAIRS(8, x, 124, 100, 60, 2, 0, 60, nullptr, nullptr, tab, tab, 0));
  REJECT("n_episodes", PAIRS(8, x, 124, 100, 60, 2, 0, 60, nullptr, nullptr, tab, tab, -2));
  REJECT("n_episodes", PAIRS(8, x, 124, 100, 60, 2, 0, 60, nullptr, nullptr, tab, tab, 101));       // more episodes than rows
  REJECT("both given", PAIRS(8, x, 124, 100, 60, 2, 0, 60, ix, nullptr, tab, tab, 4));
#undef PAIRS
  // nothing above staged a batch
  REJECT("no minibatch loaded", porl_iql_bc_step(h, &hp, nullptr));
  REJECT("no minibatch loaded", porl_iql_policy_backward(h, &hp, nullptr));
  porl_iql_destroy(h);
  for (float* p : P) std::free(p);
  std::printf("abi_reject_goal_bc: %d checks, %d unexpected\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
