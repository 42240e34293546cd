// The lidar navigation task (porl_nav_scan, porl_nav_reset, porl_nav_step): the host side of csrc/navsim.hpp.  Included
// by porl_api.hip.  Every argument is judged before the first device call; each entry point is one launch with no
// allocation and no synchronisation.

namespace {

constexpr int64_t NAV_MAX_ROBOTS = int64_t(1) << 24;
constexpr int64_t NAV_MAX_STRIDE = int64_t(1) << 24;

bool nav_pos(double v) { return std::isfinite(v) && v > 0.0; }

int nav_check_world(const float* segments, int32_t M, const float* circles, int32_t C, const double* beam_dirs,
                    const porl_nav_params* p, int64_t n) {
  if (!p) PORL_FAIL(PORL_ERR_INVALID, "null params");
  if (M < 0) PORL_FAIL(PORL_ERR_INVALID, "M %d must not be negative", M);
  if (C < 0) PORL_FAIL(PORL_ERR_INVALID, "C %d must not be negative", C);
  if ((int64_t)M + (int64_t)C > PORL_NAV_MAX_PRIMS)
    PORL_FAIL(PORL_ERR_INVALID, "M + C = %lld primitives, at most %d", (long long)M + C, PORL_NAV_MAX_PRIMS);
  if (M > 0 && !segments) PORL_FAIL(PORL_ERR_INVALID, "null segments (M = %d)", M);
  if (C > 0 && !circles) PORL_FAIL(PORL_ERR_INVALID, "null circles (C = %d)", C);
  if (!beam_dirs) PORL_FAIL(PORL_ERR_INVALID, "null beam_dirs");
  if (p->n_beams < 1 || p->n_beams > PORL_NAV_MAX_BEAMS)
    PORL_FAIL(PORL_ERR_INVALID, "n_beams %d outside [1, %d]", p->n_beams, PORL_NAV_MAX_BEAMS);
  if (!nav_pos(p->range_max)) PORL_FAIL(PORL_ERR_INVALID, "range_max must be positive and finite");
  if (!std::isfinite(p->no_return)) PORL_FAIL(PORL_ERR_INVALID, "no_return must be finite");
  if (p->layout != PORL_NAV_LAYOUT_GOAL && p->layout != PORL_NAV_LAYOUT_POSE)
    PORL_FAIL(PORL_ERR_INVALID, "layout %d is neither PORL_NAV_LAYOUT_GOAL nor PORL_NAV_LAYOUT_POSE", p->layout);
  if (p->reserved) PORL_FAIL(PORL_ERR_INVALID, "reserved must be 0");
  if (n < 1 || n > NAV_MAX_ROBOTS) PORL_FAIL(PORL_ERR_INVALID, "n %lld outside [1, 2^24]", (long long)n);
  return PORL_OK;
}

// what reset and step need beyond the cast
int nav_check_task(const porl_nav_params* p, const double* state, const int64_t* counters, const float* obs, int64_t obs_stride) {
  if (!nav_pos(p->dt) || p->dt > 10.0) PORL_FAIL(PORL_ERR_INVALID, "dt outside (0, 10]");
  if (!(p->max_lin_vel >= 0.0) || !std::isfinite(p->max_lin_vel)) PORL_FAIL(PORL_ERR_INVALID, "max_lin_vel must be finite and not negative");
  if (!(p->max_ang_vel >= 0.0) || !std::isfinite(p->max_ang_vel)) PORL_FAIL(PORL_ERR_INVALID, "max_ang_vel must be finite and not negative");
  if (!nav_pos(p->min_range)) PORL_FAIL(PORL_ERR_INVALID, "min_range must be positive and finite");
  if (!(p->max_lin_vel * p->dt < p->min_range))
    PORL_FAIL(PORL_ERR_INVALID, "max_lin_vel * dt must stay below min_range: a robot could pass a wall between two scans");
  if (!(p->max_ang_vel * p->dt < 3.141592653589793)) PORL_FAIL(PORL_ERR_INVALID, "max_ang_vel * dt must stay below pi");
  if (!(p->goal_radius >= 0.0) || !std::isfinite(p->goal_radius)) PORL_FAIL(PORL_ERR_INVALID, "goal_radius must be finite and not negative");
  if (!std::isfinite(p->hit_reward)) PORL_FAIL(PORL_ERR_INVALID, "hit_reward must be finite");
  if (!std::isfinite(p->goal_reward)) PORL_FAIL(PORL_ERR_INVALID, "goal_reward must be finite");
  if (!std::isfinite(p->origin_x) || !std::isfinite(p->origin_y)) PORL_FAIL(PORL_ERR_INVALID, "origin_x / origin_y must be finite");
  if (!std::isfinite(p->spawn_lo) || !std::isfinite(p->spawn_span) || p->spawn_span < 0.0)
    PORL_FAIL(PORL_ERR_INVALID, "spawn_lo / spawn_span must be finite, spawn_span not negative");
  if (!std::isfinite(p->min_gap_sq)) PORL_FAIL(PORL_ERR_INVALID, "min_gap_sq must be finite");
  if (!std::isfinite(p->goal_dist_lo) || !std::isfinite(p->goal_dist_hi) || !(p->goal_dist_lo <= p->goal_dist_hi))
    PORL_FAIL(PORL_ERR_INVALID, "goal_dist_lo / goal_dist_hi must be finite and ordered");
  if (p->episode_step < 1) PORL_FAIL(PORL_ERR_INVALID, "episode_step %d must be positive", p->episode_step);
  if (p->cells < 1 || p->cells > (1 << 20)) PORL_FAIL(PORL_ERR_INVALID, "cells %d outside [1, 2^20]", p->cells);
  if (!state) PORL_FAIL(PORL_ERR_INVALID, "null state");
  if (!counters) PORL_FAIL(PORL_ERR_INVALID, "null counters");
  if (!obs) PORL_FAIL(PORL_ERR_INVALID, "null obs");
  const int S = p->n_beams + (p->layout ? 5 : 2);
  if (obs_stride < S || obs_stride > NAV_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "obs_stride %lld: an observation is %d floats", (long long)obs_stride, S);
  return PORL_OK;
}

size_t nav_lds_bytes(int32_t M, int32_t C, const porl_nav_params* p) { return (size_t)(M + C) * 16 + (size_t)p->n_beams * 4; }

}  // namespace

extern "C" {

int porl_nav_scan(const float* segments, int32_t M, const float* circles, int32_t C, const double* poses,
                  const double* beam_dirs, const porl_nav_params* params, float* out, int64_t out_stride, int64_t n,
                  void* stream) {
  PORL_TRY(nav_check_world(segments, M, circles, C, beam_dirs, params, n));
  if (!poses) PORL_FAIL(PORL_ERR_INVALID, "null poses");
  if (!out) PORL_FAIL(PORL_ERR_INVALID, "null out");
  if (out_stride < params->n_beams || out_stride > NAV_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "out_stride %lld: a scan is n_beams = %d floats", (long long)out_stride, params->n_beams);
  DevGuard _dg(device_of(out));
  const NavWorldArgs w{segments, M, circles, C, beam_dirs};
  hipLaunchKernelGGL(nav_scan_kernel, dim3((unsigned)n), dim3(NAV_THREADS), nav_lds_bytes(M, C, params), (hipStream_t)stream, w,
                     *params, poses, out, (long long)out_stride);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_nav_reset(const float* segments, int32_t M, const float* circles, int32_t C, const double* beam_dirs,
                   const porl_nav_params* params, uint64_t seed, int64_t env_offset, const uint8_t* mask, double* state,
                   int64_t* counters, float* obs, int64_t obs_stride, int64_t n, void* stream) {
  PORL_TRY(nav_check_world(segments, M, circles, C, beam_dirs, params, n));
  PORL_TRY(nav_check_task(params, state, counters, obs, obs_stride));
  if (env_offset < 0 || env_offset > (int64_t(1) << 40)) PORL_FAIL(PORL_ERR_INVALID, "env_offset %lld outside [0, 2^40]", (long long)env_offset);
  DevGuard _dg(device_of(state));
  const NavWorldArgs w{segments, M, circles, C, beam_dirs};
  hipLaunchKernelGGL(nav_reset_kernel, dim3((unsigned)n), dim3(NAV_THREADS), nav_lds_bytes(M, C, params), (hipStream_t)stream, w,
                     *params, seed, (long long)env_offset, mask, state, reinterpret_cast<long long*>(counters), obs,
                     (long long)obs_stride);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

int porl_nav_step(const float* segments, int32_t M, const float* circles, int32_t C, const double* beam_dirs,
                  const porl_nav_params* params, uint64_t seed, int64_t env_offset, const float* actions,
                  int64_t act_stride, double* state, int64_t* counters, float* obs, int64_t obs_stride, float* next_obs,
                  int64_t next_stride, float* reward, int32_t* flags, int32_t* status, float* rows, int64_t row_stride,
                  int64_t n, void* stream) {
  PORL_TRY(nav_check_world(segments, M, circles, C, beam_dirs, params, n));
  PORL_TRY(nav_check_task(params, state, counters, obs, obs_stride));
  if (env_offset < 0 || env_offset > (int64_t(1) << 40)) PORL_FAIL(PORL_ERR_INVALID, "env_offset %lld outside [0, 2^40]", (long long)env_offset);
  const int S = params->n_beams + (params->layout ? 5 : 2);
  if (!actions) PORL_FAIL(PORL_ERR_INVALID, "null actions");
  if (act_stride < 2 || act_stride > NAV_MAX_STRIDE) PORL_FAIL(PORL_ERR_INVALID, "act_stride %lld: a command is 2 floats", (long long)act_stride);
  if (!next_obs) PORL_FAIL(PORL_ERR_INVALID, "null next_obs");
  if (next_obs == obs) PORL_FAIL(PORL_ERR_INVALID, "next_obs must not be obs (obs is read as s and rewritten)");
  if (next_stride < S || next_stride > NAV_MAX_STRIDE)
    PORL_FAIL(PORL_ERR_INVALID, "next_stride %lld: an observation is %d floats", (long long)next_stride, S);
  if (!reward) PORL_FAIL(PORL_ERR_INVALID, "null reward");
  if (!flags) PORL_FAIL(PORL_ERR_INVALID, "null flags");
  if (!status) PORL_FAIL(PORL_ERR_INVALID, "null status");
  if (rows) {
    if (row_stride < 2 * S + 4 || row_stride > NAV_MAX_STRIDE * 64)
      PORL_FAIL(PORL_ERR_INVALID, "row_stride %lld: a transition is 2 * %d + 4 floats", (long long)row_stride, S);
  } else if (row_stride != 0) {
    PORL_FAIL(PORL_ERR_INVALID, "row_stride %lld without rows (pass 0)", (long long)row_stride);
  }
  DevGuard _dg(device_of(state));
  const NavWorldArgs w{segments, M, circles, C, beam_dirs};
  NavStepArgs a{seed, (long long)env_offset, actions, (long long)act_stride, state, reinterpret_cast<long long*>(counters), obs,
                (long long)obs_stride, next_obs, (long long)next_stride, reward, flags, status, rows, (long long)row_stride};
  hipLaunchKernelGGL(nav_step_kernel, dim3((unsigned)n), dim3(NAV_THREADS), nav_lds_bytes(M, C, params), (hipStream_t)stream, w,
                     *params, a);
  PORL_HIP(hipGetLastError());
  return PORL_OK;
}

}  // extern "C"
