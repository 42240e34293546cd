// The lidar navigation task on the device (porl_nav_scan / porl_nav_reset / porl_nav_step): what env/gazebo.py asks of
// ROS and Gazebo, restated as a unicycle step and a 2-D ray cast against wall segments and pillars.
//
// Shape: ONE WORKGROUP PER ROBOT, NAV_THREADS = 384 lanes (six waves) so the reference's 360 beams are one pass with one
// lane per beam; more beams (up to 1024) take ceil(n_beams / 384) <= 3 passes.  The primitives are staged once per block
// into LDS exactly as they are stored — fp32 quadruples (x1 y1 x2 y2 | cx cy r 0), 16 bytes each, dynamic LDS of
// (M + C) * 16 bytes — and widened to fp64 as they are read: the widening is exact, so the kernel and an fp64 oracle
// reading the same fp32 values see the same world, and 2048 primitives stay at 32 KiB.  Every lane of a wave reads the same
// primitive at the same time (an LDS broadcast, no bank conflict).  Lane 0 does the scalar work (unicycle step, reward,
// termination, reset draws) between barriers; a robot reset in the launch is cast a second time by the same block.
//
// All geometry is fp64 and each range is rounded ONCE to fp32.  Contraction is switched off in every function below (NAV_EXACT): without fused
// multiply-adds every product, sum, quotient and square root below is the correctly rounded IEEE operation an fp64 host
// restatement performs, so only sin / cos / atan2 can differ from it (by an ulp of fp64).
//
// Every loop is bounded in the code: primitives (M + C <= NAV_MAX_PRIMS), beam passes (NAV_MAX_BEAMS / NAV_THREADS),
// NAV_MAX_DRAWS reset draws.  No global atomics, no communication between blocks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/porl_hip.h"
#include "episodes.hpp"   // ep_sm64

namespace porl {

// first statement of a function body: no fused multiply-adds in it (the pragma is scoped to the compound statement)
#define NAV_EXACT _Pragma("clang fp contract(off)")

constexpr int NAV_THREADS = 384;
constexpr int NAV_WAVES = NAV_THREADS / 64;
constexpr int NAV_MAX_BEAMS = 1024;
constexpr int NAV_MAX_PRIMS = 2048;
constexpr int NAV_MAX_DRAWS = 256;
constexpr int NAV_STATE = 8;      // doubles per robot
constexpr int NAV_COUNTERS = 4;   // int64 per robot: n_step, episode, status, draws_used
constexpr int NAV_STATUS_CAP = 256;

struct NavWorldArgs {
  const float* segments; int M;
  const float* circles; int C;
  const double* beam_dirs;        // (n_beams, 2): cos, sin of the beam's angle in the robot frame
};

__device__ __forceinline__ int nav_obs_width(const porl_nav_params& p) { return p.n_beams + (p.layout ? 5 : 2); }

// Dynamic LDS: (M + C) float4 primitives, then n_beams floats of scan.
__device__ __forceinline__ void nav_stage(const NavWorldArgs& w, float4* prims) {
  for (int k = threadIdx.x; k < w.M; k += NAV_THREADS)
    prims[k] = make_float4(w.segments[4 * k], w.segments[4 * k + 1], w.segments[4 * k + 2], w.segments[4 * k + 3]);
  for (int k = threadIdx.x; k < w.C; k += NAV_THREADS)
    prims[w.M + k] = make_float4(w.circles[3 * k], w.circles[3 * k + 1], w.circles[3 * k + 2], 0.f);
}

// One beam against every primitive: the smallest t with 0 < t < range_max, else range_max or more.
__device__ __forceinline__ double nav_cast_beam(const float4* prims, int M, int C, double px, double py, double dx, double dy,
                                                double range_max) {
  NAV_EXACT
  double best = range_max;
  for (int k = 0; k < M; ++k) {
    const float4 q = prims[k];
    const double ax = (double)q.x, ay = (double)q.y;
    const double ex = (double)q.z - ax, ey = (double)q.w - ay;
    const double wx = ax - px, wy = ay - py;
    const double den = dx * ey - dy * ex;
    if (den != 0.0) {
      const double t = (wx * ey - wy * ex) / den;
      const double s = (wx * dy - wy * dx) / den;
      if (s >= 0.0 && s <= 1.0 && t > 0.0 && t < best) best = t;
    }
  }
  for (int k = 0; k < C; ++k) {
    const float4 q = prims[M + k];
    const double fx = px - (double)q.x, fy = py - (double)q.y, r = (double)q.z;
    const double b = -(fx * dx + fy * dy);
    const double cc = (fx * fx + fy * fy) - r * r;
    const double disc = b * b - cc;
    if (disc >= 0.0) {
      const double t = b - sqrt(disc);
      if (t > 0.0 && t < best) best = t;
    }
  }
  return best;
}

// The block's scan from pose (px, py, yaw) into `scan` (LDS, n_beams floats); returns the block's minimum range to every
// lane.  Every lane of the block must call it.  `red` holds NAV_WAVES floats.
__device__ __forceinline__ float nav_cast_block(const NavWorldArgs& w, const porl_nav_params& p, const float4* prims,
                                                double px, double py, double yaw, float* scan, float* red) {
  NAV_EXACT
  double sy, cy;
  sincos(yaw, &sy, &cy);
  float mn = __builtin_inff();
  for (int b = threadIdx.x; b < p.n_beams; b += NAV_THREADS) {
    const double c = w.beam_dirs[2 * b], s = w.beam_dirs[2 * b + 1];
    const double dx = c * cy - s * sy, dy = s * cy + c * sy;
    const double t = nav_cast_beam(prims, w.M, w.C, px, py, dx, dy, p.range_max);
    const float r = t < p.range_max ? (float)t : (float)p.no_return;
    scan[b] = r;
    mn = fminf(mn, r);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mn = fminf(mn, __shfl_xor(mn, d));
  __syncthreads();                                   // `red` may still be read from an earlier cast
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mn;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int k = 1; k < NAV_WAVES; ++k) r = fminf(r, red[k]);
  return r;
}

__device__ __forceinline__ double nav_u01(uint64_t key, long long episode, int j) {
  NAV_EXACT
  return (double)(ep_sm64(key ^ ep_sm64((uint64_t)(256 * episode + j))) >> 11) * 0x1.0p-53;
}

struct NavDraw {
  uint64_t key; long long episode; int j; int capped;
  const porl_nav_params* p;
  // randint(cells) + uniform(spawn_lo, spawn_lo + spawn_span): an integer draw, then a uniform draw
  __device__ __forceinline__ double coord(double cur) {
    NAV_EXACT
    if (j + 2 > NAV_MAX_DRAWS) { capped = 1; return cur; }
    const double k = floor((double)p->cells * nav_u01(key, episode, j));
    const double f = p->spawn_lo + p->spawn_span * nav_u01(key, episode, j + 1);
    j += 2;
    return k + f;
  }
};

// random_pts_map (env/gazebo.py:280-318) on the counter stream; one lane.  st: x y yaw gx gy prev_d prev_a 0.
__device__ __forceinline__ void nav_draw_reset(const porl_nav_params& p, uint64_t key, long long episode, double* st,
                                               long long* draws, int* capped) {
  NAV_EXACT
  NavDraw g{key, episode, 0, 0, &p};
  double x1 = 0, x2 = 0, y1 = 0, y2 = 0;
  while ((x1 - x2) * (x1 - x2) < p.min_gap_sq && !g.capped) { x1 = g.coord(x1); x2 = g.coord(x2); }
  while ((y1 - y2) * (y1 - y2) < p.min_gap_sq && !g.capped) { y1 = g.coord(y1); y2 = g.coord(y2); }
  const double X1 = p.origin_x + x1, Y1 = p.origin_y + y1;
  double X2 = p.origin_x + x2, Y2 = p.origin_y + y2;
  double dist = sqrt((Y2 - Y1) * (Y2 - Y1) + (X2 - X1) * (X2 - X1));
  while ((dist < p.goal_dist_lo || dist > p.goal_dist_hi) && !g.capped) {
    x2 = g.coord(x2); y2 = g.coord(y2);
    X2 = p.origin_x + x2; Y2 = p.origin_y + y2;
    dist = sqrt((Y2 - Y1) * (Y2 - Y1) + (X2 - X1) * (X2 - X1));
  }
  st[0] = X1; st[1] = Y1; st[2] = 0.0; st[3] = X2; st[4] = Y2;
  *draws = g.j; *capped = g.capped;
}

// getRelativeGoal (env/gazebo.py:56-75): distance, goal in the robot frame, |angle|
__device__ __forceinline__ void nav_relative_goal(const double* st, double* d, double* ang, double* rx, double* ry) {
  NAV_EXACT
  const double gx = st[3] - st[0], gy = st[4] - st[1];
  double s, c;
  sincos(st[2], &s, &c);
  *d = sqrt(gx * gx + gy * gy);
  *rx = c * gx + s * gy;
  *ry = -s * gx + c * gy;
  *ang = fabs(atan2(*ry, *rx));
}

// the tail of an observation row after the scan: "goal" layout [rx ry], "pose" layout [x y yaw gx gy]
__device__ __forceinline__ void nav_obs_tail(const porl_nav_params& p, const double* st, double rx, double ry, double* tail) {
  if (p.layout) { tail[0] = st[0]; tail[1] = st[1]; tail[2] = st[2]; tail[3] = st[3]; tail[4] = st[4]; }
  else { tail[0] = rx; tail[1] = ry; }
}

__device__ __forceinline__ float nav_obs_at(const porl_nav_params& p, const float* scan, const double* tail, int k) {
  return k < p.n_beams ? scan[k] : (float)tail[k - p.n_beams];
}

// ---- porl_nav_scan ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NAV_THREADS)
nav_scan_kernel(NavWorldArgs w, porl_nav_params p, const double* __restrict__ poses, float* __restrict__ out, long long out_stride) {
  extern __shared__ float4 nav_lds[];
  __shared__ float red[NAV_WAVES];
  float4* prims = nav_lds;
  float* scan = reinterpret_cast<float*>(nav_lds + (w.M + w.C));
  nav_stage(w, prims);
  __syncthreads();
  const long long i = blockIdx.x;
  nav_cast_block(w, p, prims, poses[3 * i], poses[3 * i + 1], poses[3 * i + 2], scan, red);
  for (int k = threadIdx.x; k < p.n_beams; k += NAV_THREADS) out[i * out_stride + k] = scan[k];
}

// ---- porl_nav_reset -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NAV_THREADS)
nav_reset_kernel(NavWorldArgs w, porl_nav_params p, uint64_t seed, long long env_offset, const uint8_t* __restrict__ mask,
                 double* __restrict__ state, long long* __restrict__ counters, float* __restrict__ obs, long long obs_stride) {
  extern __shared__ float4 nav_lds[];
  __shared__ float red[NAV_WAVES];
  __shared__ double st[NAV_STATE], tail[5];
  const long long i = blockIdx.x;
  if (mask && !mask[i]) return;                       // uniform over the block
  float4* prims = nav_lds;
  float* scan = reinterpret_cast<float*>(nav_lds + (w.M + w.C));
  nav_stage(w, prims);
  if (threadIdx.x == 0) {
    long long* cn = counters + NAV_COUNTERS * i;
    const long long episode = cn[1] + 1;
    long long draws; int capped;
    nav_draw_reset(p, ep_sm64(seed ^ ep_sm64((uint64_t)(env_offset + i))), episode, st, &draws, &capped);
    double d, ang, rx, ry;
    nav_relative_goal(st, &d, &ang, &rx, &ry);
    st[5] = d; st[6] = ang; st[7] = 0.0;
    nav_obs_tail(p, st, rx, ry, tail);
    for (int k = 0; k < NAV_STATE; ++k) state[NAV_STATE * i + k] = st[k];
    cn[0] = 0; cn[1] = episode; cn[2] = capped ? NAV_STATUS_CAP : 0; cn[3] = draws;
  }
  __syncthreads();
  nav_cast_block(w, p, prims, st[0], st[1], st[2], scan, red);
  const int S = nav_obs_width(p);
  for (int k = threadIdx.x; k < S; k += NAV_THREADS) obs[i * obs_stride + k] = nav_obs_at(p, scan, tail, k);
}

// ---- porl_nav_step ------------------------------------------------------------------------------------------------------
struct NavStepArgs {
  uint64_t seed; long long env_offset;
  const float* actions; long long act_stride;
  double* state; long long* counters;
  float* obs; long long obs_stride;
  float* next_obs; long long next_stride;
  float* reward; int* flags; int* status;
  float* rows; long long row_stride;
};

__global__ void __launch_bounds__(NAV_THREADS) nav_step_kernel(NavWorldArgs w, porl_nav_params p, NavStepArgs a) {
  NAV_EXACT
  extern __shared__ float4 nav_lds[];
  __shared__ float red[NAV_WAVES];
  __shared__ double st[NAV_STATE], tail[5], tail2[5];
  __shared__ float sh_reward, sh_act[2];
  __shared__ int sh_frozen, sh_term, sh_reset;
  float4* prims = nav_lds;
  float* scan = reinterpret_cast<float*>(nav_lds + (w.M + w.C));
  const long long i = blockIdx.x;
  const int S = nav_obs_width(p), tid = threadIdx.x;
  long long* cn = a.counters + NAV_COUNTERS * i;
  float* obs = a.obs + i * a.obs_stride;
  float* nxt = a.next_obs + i * a.next_stride;
  float* row = a.rows ? a.rows + i * a.row_stride : nullptr;
  nav_stage(w, prims);
  if (tid == 0) {
    const long long status = cn[2];
    sh_frozen = (status & 0xff) != 0;
    if (!sh_frozen) {
      for (int k = 0; k < NAV_STATE; ++k) st[k] = a.state[NAV_STATE * i + k];
      // 1. the command, clipped; a non-finite component counts as 0
      double v = (double)a.actions[i * a.act_stride], om = (double)a.actions[i * a.act_stride + 1];
      if (!isfinite(v)) v = 0.0;
      if (!isfinite(om)) om = 0.0;
      v = v < 0.0 ? 0.0 : (v > p.max_lin_vel ? p.max_lin_vel : v);
      om = om < -p.max_ang_vel ? -p.max_ang_vel : (om > p.max_ang_vel ? p.max_ang_vel : om);
      sh_act[0] = (float)v; sh_act[1] = (float)om;
      // 2. the exact arc over dt
      const double th = om * p.dt, h = th / 2.0;
      const double sinc = fabs(h) >= 1e-4 ? sin(h) / h : 1.0 - h * h / 6.0;
      const double chord = v * p.dt * sinc;
      double sd, cd;
      sincos(st[2] + h, &sd, &cd);
      st[0] = st[0] + chord * cd;
      st[1] = st[1] + chord * sd;
      double yaw = st[2] + th;
      const double PI = 3.141592653589793;
      if (yaw > PI) yaw -= 2.0 * PI;
      else if (yaw <= -PI) yaw += 2.0 * PI;
      st[2] = yaw;
    }
  }
  __syncthreads();
  if (sh_frozen) {                                    // a finished robot: nothing changes
    for (int k = tid; k < S; k += NAV_THREADS) nxt[k] = obs[k];
    if (row) for (int k = tid; k < 2 * S + 4; k += NAV_THREADS) row[k] = __builtin_nanf("");
    if (tid == 0) { a.reward[i] = 0.f; a.flags[i] = 0; a.status[i] = (int)cn[2]; }
    return;
  }
  // 3. scan at the new pose
  const float mn = nav_cast_block(w, p, prims, st[0], st[1], st[2], scan, red);
  if (tid == 0) {
    // 4. - 5. relative goal and the shaped reward
    double d, ang, rx, ry;
    nav_relative_goal(st, &d, &ang, &rx, &ry);
    double r = d < st[5] ? st[5] - d : 2.0 * (st[5] - d);
    r += ang < st[6] ? st[6] - ang : 2.0 * (st[6] - ang);
    st[5] = d; st[6] = ang;
    // 6. - 7. collision, then goal (goal wins)
    int term = 0;
    long long status = 0;
    if ((double)mn > 0.0 && (double)mn < p.min_range) { term = 1; r = p.hit_reward; status = 1; }
    if (d < p.goal_radius) { term = 1; r = p.goal_reward; status = 2; }
    // 8. the step count
    const long long n_step = cn[0] + 1;
    const int trunc = n_step >= (long long)p.episode_step;
    if (!term && trunc) status = 3;
    nav_obs_tail(p, st, rx, ry, tail);
    sh_reward = (float)r; sh_term = term;
    a.reward[i] = (float)r; a.flags[i] = term | (trunc << 1); a.status[i] = (int)status;
    cn[0] = n_step;
    sh_reset = 0;
    if ((term || trunc) && p.auto_reset) {
      sh_reset = 1;
      const long long episode = cn[1] + 1;
      long long draws; int capped;
      nav_draw_reset(p, ep_sm64(a.seed ^ ep_sm64((uint64_t)(a.env_offset + i))), episode, st, &draws, &capped);
      nav_relative_goal(st, &d, &ang, &rx, &ry);
      st[5] = d; st[6] = ang;
      nav_obs_tail(p, st, rx, ry, tail2);
      cn[0] = 0; cn[1] = episode; cn[2] = capped ? NAV_STATUS_CAP : 0; cn[3] = draws;
    } else {
      cn[2] = status;
    }
    st[7] = 0.0;
    for (int k = 0; k < NAV_STATE; ++k) a.state[NAV_STATE * i + k] = st[k];
  }
  __syncthreads();
  // 9. outputs: [s | r | s' | terminated | a], next_obs, and the observation to act on next
  const int do_reset = sh_reset;
  for (int k = tid; k < S; k += NAV_THREADS) {
    const float o = nav_obs_at(p, scan, tail, k);
    if (row) { row[k] = obs[k]; row[S + 1 + k] = o; }
    nxt[k] = o;
    if (!do_reset) obs[k] = o;
  }
  if (row && tid == 0) { row[S] = sh_reward; row[2 * S + 1] = sh_term ? 1.f : 0.f; row[2 * S + 2] = sh_act[0]; row[2 * S + 3] = sh_act[1]; }
  if (do_reset) {                                     // 10. the robot reset in this launch is cast again from its new pose
    __syncthreads();                                  // every lane is done reading `scan`
    nav_cast_block(w, p, prims, st[0], st[1], st[2], scan, red);
    for (int k = tid; k < S; k += NAV_THREADS) obs[k] = nav_obs_at(p, scan, tail2, k);
  }
}

}  // namespace porl
