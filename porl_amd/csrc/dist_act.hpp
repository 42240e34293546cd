// Acting for N robots with a distributional head (porl_dist_select, porl_qnet_act_rows_dist): the (n, A * NS) quantiles
// (QR-DQN) or atom logits (C51) of n robots become one value per action and an epsilon-greedy action per robot, on the
// device.  The single-robot form of the same rule is online_act_kernel's C51 / QR epilogue (csrc/online.hpp).
//
// The value of an action is computed in the order the loss heads rank the next state's actions by (dist_losses.hpp):
//   QR   mean_j z[a, j]                      lane-strided partial sums, xor butterfly 32..1, / (float)NS   (qr_loss_kernel)
//   C51  sum_n softmax(z[a, :])_n support_n  wave max, se = sum expf(z - mx), lse = mx + logf(se),
//                                            q = sum expf(z - lse) * support[n]; each sum as above          (c51_loss_kernel)
// so acting and bootstrapping agree on which action is best.  The action is qnet_select_kernel's rule on those values
// (navsim_discrete.hpp): the same key, the same two draws, the same arg-max (ties to the lowest index, the first NaN wins).
//
// Shape: ONE WAVE PER ROBOT ROW, four rows per 256-thread block, no LDS, no barriers.  An action's NS <= 256 values sit in
// at most four registers per lane across the passes, so a row is read once; lane-strided loads over a contiguous row
// coalesce.  The A values and the action are written every time, also when the robot explores.
#pragma once
#include "dist_losses.hpp"
#include "navsim_discrete.hpp"

namespace porl {

constexpr int DIST_ACT_REGS = DIST_MAX_N / 64;     // values of one action per lane

struct DistSelectArgs {
  const float* z; long long z_rs;        // (n, >= A * NS): action a in columns [a * NS, (a + 1) * NS)
  const float* support;                  // C51: (NS) atom values
  float* q; long long q_rs;              // (n, >= A) action values out
  long long* out;                        // (n) actions out
  long long n, env_offset, t;
  double epsilon;
  uint64_t seed;
  int kind, A, NS;                       // kind: 0 QR, 1 C51 (PORL_DIST_QR / PORL_DIST_C51)
};

__device__ __forceinline__ float dist_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float dist_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// the statements of qr_loss_kernel's next-action loop on registers
__device__ __forceinline__ float dist_value_qr(const float* v, int lane, int N) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < DIST_ACT_REGS; ++k)
    if (lane + 64 * k < N) s += v[k];
  s = dist_wave_sum(s);
  return s / (float)N;
}

// the statements of c51_loss_kernel's target-action loop on registers
__device__ __forceinline__ float dist_value_c51(const float* v, const float* __restrict__ support, int lane, int N) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < DIST_ACT_REGS; ++k)
    if (lane + 64 * k < N) mx = fmaxf(mx, v[k]);
  mx = dist_wave_max(mx);
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < DIST_ACT_REGS; ++k)
    if (lane + 64 * k < N) se += expf(v[k] - mx);
  se = dist_wave_sum(se);
  const float lse = mx + logf(se);
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < DIST_ACT_REGS; ++k)
    if (lane + 64 * k < N) q += expf(v[k] - lse) * support[lane + 64 * k];
  return dist_wave_sum(q);
}

__global__ void __launch_bounds__(256)
dist_select_kernel(const DistSelectArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + wave;
  if (i >= a.n) return;                               // uniform over the wave; the kernel has no block barrier
  const int N = a.NS, A = a.A;
  const float* __restrict__ row = a.z + i * a.z_rs;
  float best = 0.f, mine = 0.f;                       // mine: lane `act` keeps the value of action `act` (A <= 64)
  long long pick = 0;
  for (int act = 0; act < A; ++act) {
    float v[DIST_ACT_REGS];
#pragma unroll
    for (int k = 0; k < DIST_ACT_REGS; ++k) {
      const int j = lane + 64 * k;
      v[k] = j < N ? row[act * N + j] : 0.f;
    }
    const float val = a.kind == 0 ? dist_value_qr(v, lane, N) : dist_value_c51(v, a.support, lane, N);
    if (lane == act) mine = val;
    // qnet_select_kernel's arg-max: ties to the lowest index, a NaN counts as the maximum, the first NaN wins
    if (act == 0) best = val;
    else if (best == best && (val > best || val != val)) { best = val; pick = act; }
  }
  if (lane < A) a.q[i * a.q_rs + lane] = mine;
  if (lane == 0) {
    NAV_EXACT
    const uint64_t key = ep_sm64(a.seed ^ ep_sm64((uint64_t)(a.env_offset + i)));
    const double u1 = nav_u01(key, a.t, 0);
    if (u1 < a.epsilon) {
      pick = (long long)floor((double)A * nav_u01(key, a.t, 1));
      if (pick > A - 1) pick = A - 1;
    }
    a.out[i] = pick;
  }
}

}  // namespace porl
