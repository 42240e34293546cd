// Driver of tests/test_enc_replay_host.py — the rejected-argument paths of the two entry points that read a packed replay
// store in place (porl_enc_forward_rows, porl_iql_load_batch_indexed), on the HOST-ONLY sanitized build of
// csrc/porl_api.hip (-fsanitize=address,undefined), beside abi_reject.cpp.  Every call below must fail validation before
// it reaches a HIP call, so the program runs without a GPU.  Exit code 0 = every rejection was a clean error return
// with a message and the sanitizers stayed silent (they abort the process otherwise).
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
  int64_t idx[8] = {0};
  // ---- porl_iql_load_batch_indexed ------------------------------------------------------------------------------------
  // heads on raw 60-wide states regressing s' (POR): rows of 2*60 + 2 + 2 = 124 floats
  porl_iql* h = nullptr;
  porl_iql_cfg c{60, 60, 64, 2, 0, 0, 0, 128};
  ACCEPT(porl_iql_create(&c, &h));
  REJECT("null engine", porl_iql_load_batch_indexed(nullptr, 8, x, 124, 100, idx, 60, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));
  REJECT("bind", porl_iql_load_batch_indexed(h, 8, x, 124, 100, idx, 60, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));   // unbound
  const int64_t nv = porl_iql_group_floats(h, 0), np_ = porl_iql_group_floats(h, 1), nw = porl_iql_workspace_floats(h);
  // host memory standing in for device buffers: bind only records the pointers (they are never dereferenced on the host)
  float* P[11] = {mk(nv), mk(nv), mk(np_), mk(nv), mk(np_), mk(nv), mk(nv), mk(np_), mk(np_), mk(nw), mk(8)};
  porl_iql_buffers bufs{P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7], P[8], P[9], P[10]};
  ACCEPT(porl_iql_bind(h, &bufs));
  REJECT("batch", porl_iql_load_batch_indexed(h, 0, x, 124, 100, idx, 60, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));
  REJECT("batch", porl_iql_load_batch_indexed(h, 129, x, 124, 100, idx, 60, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));
  REJECT("rows", porl_iql_load_batch_indexed(h, 8, nullptr, 124, 100, idx, 60, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));
  REJECT("idx", porl_iql_load_batch_indexed(h, 8, x, 124, 100, nullptr, 60, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));
  REJECT("n_rows", porl_iql_load_batch_indexed(h, 8, x, 124, 0, idx, 60, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));
  REJECT("n_rows", porl_iql_load_batch_indexed(h, 8, x, 124, -5, idx, 60, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));
  REJECT("row_stride", porl_iql_load_batch_indexed(h, 8, x, 123, 100, idx, 60, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));
  REJECT("next_feat", porl_iql_load_batch_indexed(h, 8, x, 124, 100, idx, 60, 2, 0, 0, x, 60, nullptr, 0, nullptr));
  REJECT("obs_feat", porl_iql_load_batch_indexed(h, 8, x, 124, 100, idx, 60, 2, 0, 0, nullptr, 0, x, 60, nullptr));
  REJECT("obs_rs", porl_iql_load_batch_indexed(h, 8, x, 124, 100, idx, 60, 2, 0, 0, x, 59, x, 60, nullptr));
  REJECT("next_rs", porl_iql_load_batch_indexed(h, 8, x, 124, 100, idx, 60, 2, 0, 0, x, 60, x, 0, nullptr));
  REJECT("state_dim", porl_iql_load_batch_indexed(h, 8, x, 200, 100, idx, 59, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));   // != obs_dim, no features
  REJECT("state_dim", porl_iql_load_batch_indexed(h, 8, x, 124, 100, idx, 0, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));
  REJECT("target", porl_iql_load_batch_indexed(h, 8, x, 124, 100, idx, 60, 2, 1, 0, nullptr, 0, nullptr, 0, nullptr));      // pol_out_dim 60 vs 2 actions
  REJECT("target", porl_iql_load_batch_indexed(h, 8, x, 800, 100, idx, 362, 2, 0, 1, x, 60, x, 60, nullptr));              // pol_out_dim 60 vs s' of 362
  REJECT("batch", porl_iql_load_batch_indexed(h, -1, x, 124, 100, idx, 60, 2, 0, 0, nullptr, 0, nullptr, 0, nullptr));
  porl_iql_destroy(h);
  for (float* p : P) std::free(p);
  // heads on 64 encoder features, SORL target (2 actions) on rows of 86-wide raw states: 2*86 + 2 + 2 = 176 floats
  porl_iql_cfg cs{64, 2, 64, 2, 0, 1, 1, 16};
  ACCEPT(porl_iql_create(&cs, &h));
  const int64_t nv2 = porl_iql_group_floats(h, 0), np2 = porl_iql_group_floats(h, 1), nw2 = porl_iql_workspace_floats(h);
  float* Q[11] = {mk(nv2), mk(nv2), mk(np2), mk(nv2), mk(np2), mk(nv2), mk(nv2), mk(np2), mk(np2), mk(nw2), mk(8)};
  porl_iql_buffers bufs2{Q[0], Q[1], Q[2], Q[3], Q[4], Q[5], Q[6], Q[7], Q[8], Q[9], Q[10]};
  ACCEPT(porl_iql_bind(h, &bufs2));
  REJECT("state_dim", porl_iql_load_batch_indexed(h, 8, x, 176, 100, idx, 86, 2, 1, 0, nullptr, 0, nullptr, 0, nullptr));  // raw rows need features
  REJECT("row_stride", porl_iql_load_batch_indexed(h, 8, x, 175, 100, idx, 86, 2, 1, 0, x, 64, x, 64, nullptr));
  REJECT("obs_rs", porl_iql_load_batch_indexed(h, 8, x, 176, 100, idx, 86, 2, 1, 0, x, 63, x, 64, nullptr));
  REJECT("target", porl_iql_load_batch_indexed(h, 8, x, 177, 100, idx, 86, 3, 1, 0, x, 64, x, 64, nullptr));
  REJECT("batch", porl_iql_load_batch_indexed(h, 17, x, 176, 100, idx, 86, 2, 1, 0, x, 64, x, 64, nullptr));
  porl_iql_destroy(h);
  for (float* p : Q) std::free(p);
  // ---- porl_enc_forward_rows ----------------------------------------------------------------------------------------------
  porl_enc* e = nullptr;
  porl_enc_cfg ec{};
  ec.n_ang = 84; ec.n_dist = 84; ec.embed_dim = 96; ec.depth0 = 1; ec.depth1 = 2; ec.n_div = 4; ec.feature_dim = 1280;
  ec.num_classes = 64; ec.max_batch = 4; ec.mlp_ratio = 2.f; ec.bn_eps = 1e-5f; ec.bn_momentum = 0.1f; ec.bf16_operands = 0;
  ACCEPT(porl_enc_create(&ec, &e));
  REJECT("null engine", porl_enc_forward_rows(nullptr, x, 176, 100, idx, 0, 2, 1, nullptr, x, 64, nullptr));
  REJECT("bind", porl_enc_forward_rows(e, x, 176, 100, idx, 0, 2, 1, nullptr, x, 64, nullptr));             // unbound
  float* ep = mk(porl_enc_param_floats(e));
  float* es = mk(porl_enc_stat_floats(e));
  float* ew = mk(porl_enc_workspace_floats(e));
  ACCEPT(porl_enc_bind(e, ep, es, ew));
  REJECT("rows", porl_enc_forward_rows(e, nullptr, 176, 100, idx, 0, 2, 1, nullptr, x, 64, nullptr));
  REJECT("idx", porl_enc_forward_rows(e, x, 176, 100, nullptr, 0, 2, 1, nullptr, x, 64, nullptr));
  REJECT("features", porl_enc_forward_rows(e, x, 176, 100, idx, 0, 2, 1, nullptr, nullptr, 64, nullptr));
  REJECT("batch", porl_enc_forward_rows(e, x, 176, 100, idx, 0, 0, 1, nullptr, x, 64, nullptr));
  REJECT("batch", porl_enc_forward_rows(e, x, 176, 100, idx, 0, 5, 1, nullptr, x, 64, nullptr));            // > max_batch
  REJECT("batch", porl_enc_forward_rows(e, x, 176, 100, idx, 0, -2, 1, nullptr, x, 64, nullptr));
  REJECT("n_rows", porl_enc_forward_rows(e, x, 176, 0, idx, 0, 2, 1, nullptr, x, 64, nullptr));
  REJECT("col_offset", porl_enc_forward_rows(e, x, 176, 100, idx, -1, 2, 1, nullptr, x, 64, nullptr));
  REJECT("col_offset", porl_enc_forward_rows(e, x, 176, 100, idx, 91, 2, 1, nullptr, x, 64, nullptr));      // 91 + 86 > 176
  REJECT("col_offset", porl_enc_forward_rows(e, x, 85, 100, idx, 0, 2, 1, nullptr, x, 64, nullptr));        // the row is shorter than a state
  REJECT("col_offset", porl_enc_forward_rows(e, x, 176, 100, idx, INT32_MAX, 2, 1, nullptr, x, 64, nullptr));
  REJECT("feat_rs", porl_enc_forward_rows(e, x, 176, 100, idx, 0, 2, 1, nullptr, x, 63, nullptr));
  // the two legal offsets of a 176-wide row pass validation only with a device: not called here
  porl_enc_destroy(e);
  std::free(ep); std::free(es); std::free(ew);
  std::printf("abi_reject_rows: %d checks, %d unexpected\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
