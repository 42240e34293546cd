// Acting for N robots under discrete BCQ's constraint (porl_bcq_select, porl_qnet_act_rows_bcq): the action the learn
// step's target assumes — argmax_a [Q(s, a) + (mask(s, a) - 1) * 1e10] with mask = softmax(pi_b(s)) > threshold
// (reference src/porl/policy/bcq.py:59-72) — taken for every robot from its row of action values q (n, A) and of behaviour
// logits z (n, A), in one launch and without a read-back.
//
// One thread per robot, SELECT_THREADS per block, like qnet_select_kernel: a row is 2 * A floats (A <= 64) and the launch
// is latency-bound at the loop's sizes.  Nothing is kept per thread but scalars — the logits are read three times (maximum,
// sum, probabilities), the second and third time from cache — so the kernel holds no array and no scratch.
//
//   softmax   softmax_mask_kernel's order and expressions (kernels.hpp): mx by fmaxf over ascending j, se += expf(z[j] - mx)
//             over ascending j, p_j = expf(z[j] - mx) / se — the same bits as porl_softmax_mask on the same logits;
//   mask      allowed_j = p_j > threshold; written as 0 / 1 fp32 into the dense (n, A) `mask` when that is not null, also
//             for a robot that explores;
//   explore   qnet_select_kernel's key and draws: u1, u2 = draws 0, 1 of act-step t of robot env_offset + i; u1 < epsilon:
//             floor(A * u2), clamped — uniform over ALL A actions, as the reference explores (no constraint);
//   greedy    arg-max of v_j = q_j + (mask_j - 1.f) * 1e10f in fp32 (the step kernel's expression, qnet_fused.hpp), first
//             maximum, qnet_select_kernel's NaN rule applied to v.  mask_j - 1 is 0 or -1, so the product is exact and v_j
//             is q_j or the one rounding of q_j - 1e10f with or without a fused multiply-add.  A row with every action
//             masked is ranked by those v_j as the learn step ranks it: |q_j| < 512 (half an ulp of 1e10f) gives every
//             v_j = -1e10f and action 0.
#pragma once
#include "navsim_discrete.hpp"   // nav_u01, ep_sm64, NAV_EXACT, SELECT_THREADS, SELECT_MAX_ACTIONS

namespace porl {

__global__ void __launch_bounds__(SELECT_THREADS)
bcq_select_kernel(const float* __restrict__ q, long long q_rs, const float* __restrict__ z, long long z_rs, int A, long long n,
                  float threshold, double epsilon, uint64_t seed, long long env_offset, long long t, float* __restrict__ mask,
                  long long* __restrict__ out) {
  NAV_EXACT
  const long long i = (long long)blockIdx.x * SELECT_THREADS + threadIdx.x;
  if (i >= n) return;
  const float* zr = z + i * z_rs;
  const float* qr = q + i * q_rs;
  float mx = -INFINITY;
  for (int j = 0; j < A; ++j) mx = fmaxf(mx, zr[j]);
  float se = 0.f;
  for (int j = 0; j < A; ++j) se += expf(zr[j] - mx);
  float* mr = mask ? mask + i * (long long)A : nullptr;
  float best = 0.f;
  long long pick = 0;
  for (int j = 0; j < A; ++j) {
    const float pj = expf(zr[j] - mx) / se;
    const float m = pj > threshold ? 1.f : 0.f;
    if (mr) mr[j] = m;
    const float v = qr[j] + (m - 1.f) * 1e10f;
    // arg-max, ties to the lowest index, a NaN counts as the maximum and the first NaN wins (qnet_select_kernel)
    if (j == 0) best = v;
    else if (best == best && (v > best || v != v)) { best = v; pick = j; }
  }
  const uint64_t key = ep_sm64(seed ^ ep_sm64((uint64_t)(env_offset + i)));
  if (nav_u01(key, t, 0) < epsilon) {
    pick = (long long)floor((double)A * nav_u01(key, t, 1));
    if (pick > A - 1) pick = A - 1;
  }
  out[i] = pick;
}

}  // namespace porl
