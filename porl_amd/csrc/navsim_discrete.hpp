// The discrete lidar navigation task on the device (porl_nav_dreset / porl_nav_dstep) and the epsilon-greedy action rule
// over a table of action values (porl_qnet_select): the reference's env/env.py — the 5-action TurtleBot task runner.py
// hands to DQN_CQL — on the ray cast, the reset draw and the counter stream of csrc/navsim.hpp, which this file includes
// and does not restate.
//
// Task (env/env.py): constant forward speed, the action picks the angular velocity w = ((A - 1) / 2 - a) * ang_step
// (:139-144); observation [scan | heading | distance] with heading and distance rounded to two decimals (:59-75, :96-102);
// collision when 0 < min(scan) < min_range, goal when the rounded distance < goal_radius, the goal wins (:92-99, :123-134);
// reward round2(5 tr) * 2^(distance / goal_distance) with tr the yaw term of :110-113, or goal_reward / hit_reward;
// truncated when the step count reaches episode_step, status timelimited then, the reward unchanged (:160-164).
// round2(x) = rint(100 x) / 100 in fp64 (Python's round(x, 2) is decimal-exact: the two differ only where 100 x lies
// within an fp64 rounding of a half).  An action index outside [0, A) is clamped into range.
//
// Shape: as nav_step_kernel — ONE WORKGROUP PER ROBOT, NAV_THREADS lanes, the world staged once in LDS, fp64 geometry with
// contraction off, lane 0 doing the scalar work between barriers, a robot reset in the launch cast a second time.  All LDS
// is dynamic: (M + C) float4 primitives | NavdShared | n_beams floats of scan, every carve offset a multiple of 16 bytes.
//
// Per robot: state (N, 8) fp64 x y yaw goal_x goal_y 0 0 goal_distance (the rounded distance at reset, :55, :228);
// counters as navsim.hpp.  Two optional outputs, written by the lanes that hold the values, no atomics, no communication
// between blocks: a replay target (robot i's transition into slot (base + i) % capacity of the five arrays of a
// porl_qnet_mirror; N <= capacity, so no two robots share a slot) and episode tallies (a running fp64 return per robot;
// at an episode's end episodes, sum of returns, goals, hits are added into the robot's row of an (N, 4) fp64 table).
#pragma once
#include "navsim.hpp"

namespace porl {

constexpr int NAVD_MAX_ACTIONS = 5;       // the reference's yaw table has five entries (env/env.py:110)
constexpr int SELECT_MAX_ACTIONS = 64;
constexpr int SELECT_THREADS = 256;

struct alignas(16) NavdShared {
  double st[NAV_STATE];
  double tail[2], tail2[2];
  float red[NAV_WAVES];
  float reward;
  int frozen, done, reset;
  long long action;
};
static_assert(sizeof(NavdShared) % 16 == 0, "the scan behind NavdShared starts on a 16-byte boundary");

__device__ __forceinline__ double navd_round2(double x) {
  NAV_EXACT
  return rint(100.0 * x) / 100.0;
}

// heading and distance of the observation's tail (getOdometry :66-75, getState :96), both rounded
__device__ __forceinline__ void navd_tail(const double* st, double* tail) {
  NAV_EXACT
  const double PI = 3.141592653589793;
  const double gx = st[3] - st[0], gy = st[4] - st[1];
  double heading = atan2(gy, gx) - st[2];
  if (heading > PI) heading -= 2.0 * PI;
  else if (heading < -PI) heading += 2.0 * PI;
  tail[0] = navd_round2(heading);
  tail[1] = navd_round2(sqrt(gx * gx + gy * gy));
}

// setReward :104-116 without the terminal branches; `%` is Python's (non-negative for a positive divisor)
__device__ __forceinline__ double navd_shaped_reward(double heading, double distance, double goal_distance, long long a) {
  NAV_EXACT
  const double PI = 3.141592653589793;
  const double angle = -PI / 4.0 + heading + PI / 8.0 * (double)a + PI / 2.0;
  double m = fmod(0.5 * angle, 2.0 * PI);
  if (m < 0.0) m += 2.0 * PI;
  if (m == 0.0) m = 0.0;                               // -0 reads +0, as Python's % returns it
  const double v = 0.25 + m / PI;
  const double tr = 1.0 - 4.0 * fabs(0.5 - (v - floor(v)));
  return navd_round2(tr * 5.0) * exp2(distance / goal_distance);
}

// the exact arc over dt, as step 2 of nav_step_kernel
__device__ __forceinline__ void navd_move(const porl_nav_params& p, double v, double om, double* st) {
  NAV_EXACT
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

// a new episode of robot i on lane 0: start, goal, goal_distance, counters; the tail of its first observation
__device__ __forceinline__ void navd_respawn(const porl_nav_params& p, uint64_t seed, long long env, long long* cn, double* st,
                                             double* tail) {
  const long long episode = cn[1] + 1;
  long long draws; int capped;
  nav_draw_reset(p, ep_sm64(seed ^ ep_sm64((uint64_t)env)), episode, st, &draws, &capped);
  st[5] = 0.0; st[6] = 0.0;
  navd_tail(st, tail);
  st[7] = tail[1];
  cn[0] = 0; cn[1] = episode; cn[2] = capped ? NAV_STATUS_CAP : 0; cn[3] = draws;
}

__device__ __forceinline__ float navd_obs_at(int n_beams, const float* scan, const double* tail, int k) {
  return k < n_beams ? scan[k] : (float)tail[k - n_beams];
}

__device__ __forceinline__ NavdShared* navd_carve(float4* lds, int n_prims, float** scan) {
  NavdShared* sh = reinterpret_cast<NavdShared*>(lds + n_prims);
  *scan = reinterpret_cast<float*>(sh + 1);
  return sh;
}

// ---- porl_nav_dreset ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NAV_THREADS)
navd_reset_kernel(NavWorldArgs w, porl_nav_params p, uint64_t seed, long long env_offset, const uint8_t* __restrict__ mask,
                  double* __restrict__ state, long long* __restrict__ counters, float* __restrict__ obs, long long obs_stride,
                  double* __restrict__ returns) {
  extern __shared__ float4 nav_lds[];
  const long long i = blockIdx.x;
  if (mask && !mask[i]) return;                       // uniform over the block
  float* scan;
  NavdShared* sh = navd_carve(nav_lds, w.M + w.C, &scan);
  nav_stage(w, nav_lds);
  if (threadIdx.x == 0) {
    navd_respawn(p, seed, env_offset + i, counters + NAV_COUNTERS * i, sh->st, sh->tail);
    for (int k = 0; k < NAV_STATE; ++k) state[NAV_STATE * i + k] = sh->st[k];
    if (returns) returns[i] = 0.0;
  }
  __syncthreads();
  nav_cast_block(w, p, nav_lds, sh->st[0], sh->st[1], sh->st[2], scan, sh->red);
  const int S = p.n_beams + 2;
  for (int k = threadIdx.x; k < S; k += NAV_THREADS) obs[i * obs_stride + k] = navd_obs_at(p.n_beams, scan, sh->tail, k);
}

// ---- porl_nav_dstep -----------------------------------------------------------------------------------------------------
struct NavdStepArgs {
  uint64_t seed; long long env_offset;
  const long long* actions;
  double* state; long long* counters;
  float* obs; long long obs_stride;
  float* next_obs; long long next_stride;
  float* reward; int* flags; int* status;
  // replay target (r_states == nullptr: none): dense rows of S floats, slot (r_base + i) % r_capacity
  float* r_states; float* r_next; long long* r_actions; float* r_rewards; float* r_dones;
  long long r_capacity, r_base;
  // episode tallies (nullptr: none): (N, 4) fp64 episodes, sum of returns, goals, hits; returns (N) the running return
  double* tallies; double* returns;
};

// (8 waves per SIMD: five blocks to a CU, as nav_step_kernel has them; the scalar section of lane 0 would otherwise take
// the kernel to 67 VGPRs and four blocks)
__global__ void __launch_bounds__(NAV_THREADS, 8)
navd_step_kernel(NavWorldArgs w, porl_nav_params p, porl_nav_discrete d, NavdStepArgs a) {
  NAV_EXACT
  extern __shared__ float4 nav_lds[];
  float* scan;
  NavdShared* sh = navd_carve(nav_lds, w.M + w.C, &scan);
  const long long i = blockIdx.x;
  const int S = p.n_beams + 2, tid = threadIdx.x;
  long long* cn = a.counters + NAV_COUNTERS * i;
  float* obs = a.obs + i * a.obs_stride;
  float* nxt = a.next_obs + i * a.next_stride;
  nav_stage(w, nav_lds);
  if (tid == 0) {
    sh->frozen = (cn[2] & 0xff) != 0;
    if (!sh->frozen) {
      for (int k = 0; k < NAV_STATE; ++k) sh->st[k] = a.state[NAV_STATE * i + k];
      // 1. the command of the clamped action index (:139-144)
      long long act = a.actions[i];
      act = act < 0 ? 0 : (act > (long long)d.n_actions - 1 ? (long long)d.n_actions - 1 : act);
      sh->action = act;
      const double om = ((double)(d.n_actions - 1) / 2.0 - (double)act) * d.ang_step;
      // 2. the exact arc over dt
      navd_move(p, d.lin_vel, om, sh->st);
    }
  }
  __syncthreads();
  if (sh->frozen) {                                   // a finished robot: nothing changes, nothing is recorded
    for (int k = tid; k < S; k += NAV_THREADS) nxt[k] = obs[k];
    if (tid == 0) { a.reward[i] = 0.f; a.flags[i] = 0; a.status[i] = (int)cn[2]; }
    return;
  }
  // 3. scan at the new pose
  const float mn = nav_cast_block(w, p, nav_lds, sh->st[0], sh->st[1], sh->st[2], scan, sh->red);
  if (tid == 0) {
    double* st = sh->st;
    // 4. heading and distance, rounded: what the agent observes and what the reward reads
    navd_tail(st, sh->tail);
    const double heading = sh->tail[0], dist = sh->tail[1];
    // 5. collision, then goal (the goal wins), else the shaped reward
    const int hit = (double)mn > 0.0 && (double)mn < p.min_range;
    const int goal = dist < p.goal_radius;
    const int term = hit | goal;
    double r = navd_shaped_reward(heading, dist, st[7], sh->action);
    long long status = 0;
    if (term) { r = goal ? d.goal_reward : d.hit_reward; status = goal ? 2 : 1; }
    // 6. the step count; the reward is not altered by truncation
    const long long n_step = cn[0] + 1;
    const int trunc = n_step >= (long long)p.episode_step;
    if (trunc) status = 3;
    const float rf = (float)r;
    sh->reward = rf; sh->done = term | trunc;
    a.reward[i] = rf; a.flags[i] = term | (trunc << 1); a.status[i] = (int)status;
    if (a.tallies) {
      const double ret = a.returns[i] + (double)rf;
      if (term | trunc) {
        double* ta = a.tallies + 4 * i;
        ta[0] = ta[0] + 1.0; ta[1] = ta[1] + ret;
        ta[2] = ta[2] + (goal ? 1.0 : 0.0); ta[3] = ta[3] + (hit && !goal ? 1.0 : 0.0);
        a.returns[i] = 0.0;
      } else {
        a.returns[i] = ret;
      }
    }
    cn[0] = n_step;
    sh->reset = 0;
    if ((term || trunc) && p.auto_reset) {
      sh->reset = 1;
      navd_respawn(p, a.seed, a.env_offset + i, cn, st, sh->tail2);
    } else {
      cn[2] = status;
    }
    for (int k = 0; k < NAV_STATE; ++k) a.state[NAV_STATE * i + k] = st[k];
  }
  __syncthreads();
  // 7. outputs: next_obs, the replay slot, and the observation to act on next
  const int do_reset = sh->reset;
  const long long slot = a.r_states ? (a.r_base + i) % a.r_capacity : 0;
  float* rs = a.r_states ? a.r_states + slot * S : nullptr;
  float* rn = a.r_states ? a.r_next + slot * S : nullptr;
  for (int k = tid; k < S; k += NAV_THREADS) {
    const float o = navd_obs_at(p.n_beams, scan, sh->tail, k);
    if (rs) { rs[k] = obs[k]; rn[k] = o; }
    nxt[k] = o;
    if (!do_reset) obs[k] = o;
  }
  if (rs && tid == 0) {
    a.r_actions[slot] = sh->action; a.r_rewards[slot] = sh->reward; a.r_dones[slot] = sh->done ? 1.f : 0.f;
  }
  if (do_reset) {                                     // 8. the robot reset in this launch is cast again from its new pose
    __syncthreads();                                  // every lane is done reading `scan`
    nav_cast_block(w, p, nav_lds, sh->st[0], sh->st[1], sh->st[2], scan, sh->red);
    for (int k = tid; k < S; k += NAV_THREADS) obs[k] = navd_obs_at(p.n_beams, scan, sh->tail2, k);
  }
}

// ---- porl_qnet_select ---------------------------------------------------------------------------------------------------
// One thread per robot.  u1, u2 = draws 0, 1 of "episode" t of robot env_offset + i's counter stream (nav_u01).
__global__ void __launch_bounds__(SELECT_THREADS)
qnet_select_kernel(const float* __restrict__ q, long long q_rs, int A, long long n, double epsilon, uint64_t seed,
                   long long env_offset, long long t, long long* __restrict__ out) {
  NAV_EXACT
  const long long i = (long long)blockIdx.x * SELECT_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = ep_sm64(seed ^ ep_sm64((uint64_t)(env_offset + i)));
  const double u1 = nav_u01(key, t, 0);
  long long pick;
  if (u1 < epsilon) {
    pick = (long long)floor((double)A * nav_u01(key, t, 1));
    if (pick > A - 1) pick = A - 1;
  } else {
    // arg-max, ties to the lowest index, a NaN counts as the maximum (torch.argmax)
    const float* row = q + i * q_rs;
    float best = row[0];
    pick = 0;
    for (int j = 1; j < A; ++j) {
      const float v = row[j];
      if (best == best && (v > best || v != v)) { best = v; pick = j; }
    }
  }
  out[i] = pick;
}

}  // namespace porl
