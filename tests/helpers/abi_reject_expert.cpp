// Driver of tests/test_expert_host.py — the rejected-argument paths of the A* expert's entry points (porl_nav_rasterize,
// porl_nav_expert) on the HOST-ONLY sanitized build of csrc/porl_api.hip (-fsanitize=address,undefined), beside
// abi_reject_navsim.cpp.  Every call below must fail validation before it reaches a HIP call, so the program makes no
// launch and runs without a GPU.  Exit code 0 = every rejection was a clean error return with a message that names the
// argument and the sanitizers stayed silent (they abort the process otherwise).
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

int main() {
  if (porl_abi_version() != PORL_ABI_VERSION) return 2;
  // host memory standing in for device buffers: every call is refused before anything would touch them
  static float seg[16], cir[48], cmd[8], sco[4 * 64];
  static double state[32], wp[8];
  static uint32_t bits[128], field[4 * 2809];
  static int64_t tag[4];
  static int32_t plen[4], sta[4], path[4 * 2 * 8];
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const porl_nav_grid gd{0.1, 0.18, -10.0, 5.0, 51, 51};
  const porl_nav_expert_params pd{0.2, 0.15, 1.5, 0.75, 5, 2, 8, 0};
  porl_nav_grid g = gd;
  porl_nav_expert_params p = pd;
#define RAST(seg_, M, cir_, C, gp, bm, nw) porl_nav_rasterize(seg_, M, cir_, C, gp, bm, nw, nullptr)
#define EXPERT(gp, bm, pp, st, fl, tg, cm, cs, sc, ss, n) \
  porl_nav_expert(gp, bm, pp, st, fl, tg, cm, cs, sc, ss, wp, plen, sta, path, n, nullptr)
  // ---- porl_nav_rasterize -------------------------------------------------------------------------------------------------
  REJECT("M ", RAST(seg, -1, cir, 16, &g, bits, 88));
  REJECT("C ", RAST(seg, 4, cir, -2, &g, bits, 88));
  REJECT("primitives", RAST(seg, 2040, cir, 9, &g, bits, 88));
  REJECT("primitives", RAST(seg, INT32_MAX, cir, INT32_MAX, &g, bits, 88));
  REJECT("null segments", RAST(nullptr, 4, cir, 16, &g, bits, 88));
  REJECT("null circles", RAST(seg, 4, nullptr, 16, &g, bits, 88));
  REJECT("null grid", RAST(seg, 4, cir, 16, nullptr, bits, 88));
  REJECT("null bitmap", RAST(seg, 4, cir, 16, &g, nullptr, 88));
  REJECT("n_words", RAST(seg, 4, cir, 16, &g, bits, 87));          // 53 * 53 = 2809 cells: 88 words
  REJECT("n_words", RAST(seg, 4, cir, 16, &g, bits, -1));
  REJECT("n_words", RAST(seg, 4, cir, 16, &g, bits, INT64_MAX));
  g = gd; g.resolution = 0;    REJECT("resolution", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.resolution = -0.1; REJECT("resolution", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.resolution = nan;  REJECT("resolution", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.resolution = inf;  REJECT("resolution", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.inflate = -0.01;   REJECT("inflate", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.inflate = nan;     REJECT("inflate", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.min_x = inf;       REJECT("min_x", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.min_y = nan;       REJECT("min_y", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.w = 0;             REJECT("grid", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.h = -5;            REJECT("grid", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.w = 300; g.h = 300;              REJECT("grid", RAST(seg, 4, cir, 16, &g, bits, 88));   // 91 204 padded cells
  g = gd; g.w = 254; g.h = 254;              REJECT("LDS", RAST(seg, 4, cir, 16, &g, bits, 88));    // 65 536 cells, 270 KB of LDS
  g = gd; g.w = 65533; g.h = 2;              REJECT("grid", RAST(seg, 4, cir, 16, &g, bits, 88));
  g = gd; g.w = INT32_MAX; g.h = INT32_MAX;  REJECT("grid", RAST(seg, 4, cir, 16, &g, bits, 88));
  // ---- porl_nav_expert ----------------------------------------------------------------------------------------------------
  g = gd;
  REJECT("null grid", EXPERT(nullptr, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  REJECT("null bitmap", EXPERT(&g, nullptr, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  REJECT("null params", EXPERT(&g, bits, nullptr, state, field, tag, cmd, 2, nullptr, 0, 4));
  REJECT("null state", EXPERT(&g, bits, &p, nullptr, field, tag, cmd, 2, nullptr, 0, 4));
  REJECT("null field", EXPERT(&g, bits, &p, state, nullptr, tag, cmd, 2, nullptr, 0, 4));
  REJECT("null tag", EXPERT(&g, bits, &p, state, field, nullptr, cmd, 2, nullptr, 0, 4));
  REJECT("n ", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 0));
  REJECT("n ", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, -4));
  REJECT("n ", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, (int64_t(1) << 24) + 1));
  REJECT("cmd_stride", EXPERT(&g, bits, &p, state, field, tag, cmd, 1, nullptr, 0, 4));
  REJECT("cmd_stride", EXPERT(&g, bits, &p, state, field, tag, cmd, INT64_MAX, nullptr, 0, 4));
  REJECT("without commands", EXPERT(&g, bits, &p, state, field, tag, nullptr, 2, nullptr, 0, 4));
  REJECT("score_stride", EXPERT(&g, bits, &p, state, field, tag, nullptr, 0, sco, 4, 4));
  REJECT("score_stride", EXPERT(&g, bits, &p, state, field, tag, nullptr, 0, sco, -5, 4));
  REJECT("without scores", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 5, 4));
  p = pd; p.n_actions = 0;   REJECT("n_actions", EXPERT(&g, bits, &p, state, field, tag, nullptr, 0, sco, 5, 4));
  p = pd; p.n_actions = 65;  REJECT("n_actions", EXPERT(&g, bits, &p, state, field, tag, nullptr, 0, sco, 65, 4));
  p = pd; p.n_actions = -1;  REJECT("n_actions", EXPERT(&g, bits, &p, state, field, tag, nullptr, 0, sco, 5, 4));
  p = pd; p.ang_step = nan;  REJECT("ang_step", EXPERT(&g, bits, &p, state, field, tag, nullptr, 0, sco, 5, 4));
  p = pd; p.ang_step = -1;   REJECT("ang_step", EXPERT(&g, bits, &p, state, field, tag, nullptr, 0, sco, 5, 4));
  p = pd; p.lookahead = 0;   REJECT("lookahead", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  p = pd; p.lookahead = -3;  REJECT("lookahead", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  p = pd; p.max_path = -1;   REJECT("max_path", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  p = pd; p.reserved = 7;    REJECT("reserved", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  p = pd; p.dt = 0;          REJECT("dt", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  p = pd; p.dt = nan;        REJECT("dt", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  p = pd; p.max_lin_vel = -1;  REJECT("max_lin_vel", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  p = pd; p.max_ang_vel = inf; REJECT("max_ang_vel", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  p = pd;
  g = gd; g.resolution = 0;  REJECT("resolution", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  g = gd; g.inflate = -1;    REJECT("inflate", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  g = gd; g.w = 300; g.h = 300; REJECT("grid", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  g = gd; g.w = 40000; g.h = 30000; REJECT("grid", EXPERT(&g, bits, &p, state, field, tag, cmd, 2, nullptr, 0, 4));
  std::printf("abi_reject_expert: %d checks, %d unexpected\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}
