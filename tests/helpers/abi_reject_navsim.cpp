// Driver of tests/test_navsim_host.py — the rejected-argument paths of the navigation simulator's entry points
// (porl_nav_scan, porl_nav_reset, porl_nav_step) on the HOST-ONLY sanitized build of csrc/porl_api.hip
// (-fsanitize=address,undefined), beside abi_reject_goal_bc.cpp.  Every call below must fail validation before it reaches
// a HIP call, so the program makes no launch and runs without a GPU.  Exit code 0 = every rejection was a clean error
// return with a message that names the argument and the sanitizers stayed silent (they abort the process otherwise).
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

static porl_nav_params defaults() {
  porl_nav_params p{};
  p.dt = 0.2; p.max_lin_vel = 0.15; p.max_ang_vel = 1.5; p.min_range = 0.13; p.range_max = 3.5; p.no_return = 10.0;
  p.goal_radius = 0.2; p.hit_reward = -500; p.goal_reward = 500; p.origin_x = -10; p.origin_y = 5; p.spawn_lo = 0.16;
  p.spawn_span = 0.68; p.min_gap_sq = 0.01; p.goal_dist_lo = 0.3; p.goal_dist_hi = 3.5;
  p.n_beams = 360; p.episode_step = 500; p.cells = 5; p.layout = PORL_NAV_LAYOUT_GOAL; p.auto_reset = 0; p.reserved = 0;
  return p;
}

int main() {
  if (porl_abi_version() != PORL_ABI_VERSION) return 2;
  // host memory standing in for device buffers: every call is refused before anything would touch them
  static float seg[16], cir[48], obs[4 * 365], nxt[4 * 365], act[8], rew[4], rows[4 * 734];
  static double poses[12], dirs[2 * 1024], state[32];
  static int64_t cnt[16];
  static int32_t flg[4], sta[4];
  static uint8_t mask[4];
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const porl_nav_params d = defaults();
  porl_nav_params p = d;
#define SCAN(seg_, M, cir_, C, poses_, dirs_, pp, out_, os, n) porl_nav_scan(seg_, M, cir_, C, poses_, dirs_, pp, out_, os, n, nullptr)
#define RESET(pp, mask_, st, cn, ob, os, n, off) porl_nav_reset(seg, 4, cir, 16, dirs, pp, 1, off, mask_, st, cn, ob, os, n, nullptr)
#define STEP(pp, a, as, st, cn, ob, os, nx, ns, r, f, s, rw, rs, n) \
  porl_nav_step(seg, 4, cir, 16, dirs, pp, 1, 0, a, as, st, cn, ob, os, nx, ns, r, f, s, rw, rs, n, nullptr)
  // ---- porl_nav_scan ------------------------------------------------------------------------------------------------------
  REJECT("null params", SCAN(seg, 4, cir, 16, poses, dirs, nullptr, obs, 360, 4));
  REJECT("M ", SCAN(seg, -1, cir, 16, poses, dirs, &p, obs, 360, 4));
  REJECT("C ", SCAN(seg, 4, cir, -3, poses, dirs, &p, obs, 360, 4));
  REJECT("primitives", SCAN(seg, 2040, cir, 9, poses, dirs, &p, obs, 360, 4));
  REJECT("primitives", SCAN(seg, INT32_MAX, cir, INT32_MAX, poses, dirs, &p, obs, 360, 4));
  REJECT("null segments", SCAN(nullptr, 4, cir, 16, poses, dirs, &p, obs, 360, 4));
  REJECT("null circles", SCAN(seg, 4, nullptr, 16, poses, dirs, &p, obs, 360, 4));
  REJECT("null beam_dirs", SCAN(seg, 4, cir, 16, poses, nullptr, &p, obs, 360, 4));
  REJECT("null poses", SCAN(seg, 4, cir, 16, nullptr, dirs, &p, obs, 360, 4));
  REJECT("null out", SCAN(seg, 4, cir, 16, poses, dirs, &p, nullptr, 360, 4));
  REJECT("out_stride", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 359, 4));
  REJECT("out_stride", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, -360, 4));
  REJECT("out_stride", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, INT64_MAX, 4));
  REJECT("n ", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, 0));
  REJECT("n ", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, -2));
  REJECT("n ", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, (int64_t(1) << 24) + 1));
  p = d; p.n_beams = 0;    REJECT("n_beams", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, 4));
  p = d; p.n_beams = 1025; REJECT("n_beams", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 1025, 4));
  p = d; p.n_beams = -360; REJECT("n_beams", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, 4));
  p = d; p.range_max = 0;  REJECT("range_max", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, 4));
  p = d; p.range_max = inf; REJECT("range_max", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, 4));
  p = d; p.range_max = nan; REJECT("range_max", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, 4));
  p = d; p.no_return = nan; REJECT("no_return", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, 4));
  p = d; p.layout = 2;     REJECT("layout", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, 4));
  p = d; p.reserved = 1;   REJECT("reserved", SCAN(seg, 4, cir, 16, poses, dirs, &p, obs, 360, 4));
  // ---- porl_nav_reset -----------------------------------------------------------------------------------------------------
  p = d;
  REJECT("null params", RESET(nullptr, mask, state, cnt, obs, 362, 4, 0));
  REJECT("null state", RESET(&p, mask, nullptr, cnt, obs, 362, 4, 0));
  REJECT("null counters", RESET(&p, mask, state, nullptr, obs, 362, 4, 0));
  REJECT("null obs", RESET(&p, mask, state, cnt, nullptr, 362, 4, 0));
  REJECT("obs_stride", RESET(&p, mask, state, cnt, obs, 361, 4, 0));
  REJECT("obs_stride", RESET(&p, nullptr, state, cnt, obs, 0, 4, 0));
  REJECT("n ", RESET(&p, mask, state, cnt, obs, 362, 0, 0));
  REJECT("env_offset", RESET(&p, mask, state, cnt, obs, 362, 4, -1));
  REJECT("env_offset", RESET(&p, mask, state, cnt, obs, 362, 4, INT64_MAX));
  p = d; p.layout = PORL_NAV_LAYOUT_POSE; REJECT("obs_stride", RESET(&p, mask, state, cnt, obs, 362, 4, 0));   // 365 wide
  p = d; p.dt = 0;          REJECT("dt", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.dt = nan;        REJECT("dt", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.dt = 1.0;        REJECT("min_range", RESET(&p, mask, state, cnt, obs, 362, 4, 0));     // 0.15 m per step >= 0.13
  p = d; p.max_lin_vel = 0.65; REJECT("min_range", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.max_lin_vel = -1;   REJECT("max_lin_vel", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.max_ang_vel = inf;  REJECT("max_ang_vel", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.max_ang_vel = 16;   REJECT("pi", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.min_range = 0;      REJECT("min_range", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.goal_radius = nan;  REJECT("goal_radius", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.hit_reward = inf;   REJECT("hit_reward", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.goal_reward = nan;  REJECT("goal_reward", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.origin_x = inf;     REJECT("origin_x", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.spawn_span = -0.1;  REJECT("spawn_span", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.min_gap_sq = nan;   REJECT("min_gap_sq", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.goal_dist_lo = 4;   REJECT("goal_dist_lo", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.episode_step = 0;   REJECT("episode_step", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  p = d; p.cells = 0;          REJECT("cells", RESET(&p, mask, state, cnt, obs, 362, 4, 0));
  // ---- porl_nav_step ------------------------------------------------------------------------------------------------------
  p = d;
  REJECT("null params", STEP(nullptr, act, 2, state, cnt, obs, 362, nxt, 362, rew, flg, sta, rows, 728, 4));
  REJECT("null actions", STEP(&p, nullptr, 2, state, cnt, obs, 362, nxt, 362, rew, flg, sta, rows, 728, 4));
  REJECT("act_stride", STEP(&p, act, 1, state, cnt, obs, 362, nxt, 362, rew, flg, sta, rows, 728, 4));
  REJECT("act_stride", STEP(&p, act, -2, state, cnt, obs, 362, nxt, 362, rew, flg, sta, rows, 728, 4));
  REJECT("null state", STEP(&p, act, 2, nullptr, cnt, obs, 362, nxt, 362, rew, flg, sta, rows, 728, 4));
  REJECT("null counters", STEP(&p, act, 2, state, nullptr, obs, 362, nxt, 362, rew, flg, sta, rows, 728, 4));
  REJECT("null obs", STEP(&p, act, 2, state, cnt, nullptr, 362, nxt, 362, rew, flg, sta, rows, 728, 4));
  REJECT("obs_stride", STEP(&p, act, 2, state, cnt, obs, 300, nxt, 362, rew, flg, sta, rows, 728, 4));
  REJECT("null next_obs", STEP(&p, act, 2, state, cnt, obs, 362, nullptr, 362, rew, flg, sta, rows, 728, 4));
  REJECT("next_obs must not be obs", STEP(&p, act, 2, state, cnt, obs, 362, obs, 362, rew, flg, sta, rows, 728, 4));
  REJECT("next_stride", STEP(&p, act, 2, state, cnt, obs, 362, nxt, 361, rew, flg, sta, rows, 728, 4));
  REJECT("null reward", STEP(&p, act, 2, state, cnt, obs, 362, nxt, 362, nullptr, flg, sta, rows, 728, 4));
  REJECT("null flags", STEP(&p, act, 2, state, cnt, obs, 362, nxt, 362, rew, nullptr, sta, rows, 728, 4));
  REJECT("null status", STEP(&p, act, 2, state, cnt, obs, 362, nxt, 362, rew, flg, nullptr, rows, 728, 4));
  REJECT("row_stride", STEP(&p, act, 2, state, cnt, obs, 362, nxt, 362, rew, flg, sta, rows, 727, 4));
  REJECT("row_stride", STEP(&p, act, 2, state, cnt, obs, 362, nxt, 362, rew, flg, sta, rows, 0, 4));
  REJECT("row_stride", STEP(&p, act, 2, state, cnt, obs, 362, nxt, 362, rew, flg, sta, rows, INT64_MAX, 4));
  REJECT("without rows", STEP(&p, act, 2, state, cnt, obs, 362, nxt, 362, rew, flg, sta, nullptr, 728, 4));
  REJECT("n ", STEP(&p, act, 2, state, cnt, obs, 362, nxt, 362, rew, flg, sta, rows, 728, 0));
  p = d; p.layout = PORL_NAV_LAYOUT_POSE;
  REJECT("row_stride", STEP(&p, act, 2, state, cnt, obs, 365, nxt, 365, rew, flg, sta, rows, 728, 4));     // 734 wide
  p = d; p.dt = 1.0;
  REJECT("min_range", STEP(&p, act, 2, state, cnt, obs, 362, nxt, 362, rew, flg, sta, rows, 728, 4));
  p = d; p.n_beams = 2000;
  REJECT("n_beams", STEP(&p, act, 2, state, cnt, obs, 2002, nxt, 2002, rew, flg, sta, nullptr, 0, 4));
  std::printf("abi_reject_navsim: %d checks, %d unexpected\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
