// Behaviour mask of discrete BCQ straight from the replay rows, in one launch (reference src/porl/policy/bcq.py:59-63,
// src/porl/net/behavior_policy.py:41-55):  mask[b, j] = softmax(pi_b(next_states[row(b)]))[j] > threshold ? 1 : 0,
// row(b) = idx[b], or the keyed permutation of porl_sample_indices (kernels.hpp: feistel_index) — the rows the two-group
// step kernel draws from the same (n_rows, seed, draw), so both kernels see one minibatch without an index tensor.
// Replaces gather + one launch per layer (porl_qnet_forward) + porl_softmax_mask.
//
// Built from the step kernel's pieces (qnet_fused.hpp): a block keeps 32 rows' input and activations in LDS and walks
// the layers itself on v_mfma_f32_32x32x2_f32; a layer's weights are the engine's padded image, fetched into registers
// while the layer before it is computed (qf_fetch_w / qf_park_w), barriers retire LDS traffic only (qf_barrier).  The
// softmax is the arithmetic of softmax_mask_kernel (kernels.hpp) in the same order, so the two masks agree wherever no
// probability sits within rounding of the threshold (the logits differ in summation order only).
#pragma once
#include "kernels.hpp"
#include "qnet_fused.hpp"

namespace porl {

struct BcqMaskArgs {
  const float* params;               // behaviour network, flat image layout (porl_qnet_create)
  const float* next_states; long n_rs;
  const int64_t* idx;                // (B,) source rows; unused when samp_n > 0
  float* mask;                       // (B, n_actions) by minibatch position
  int B, n_lin;
  int dims[QF_MAX_LIN + 1];
  long w_off[QF_MAX_LIN];
  // LDS offsets (floats, multiples of 4): source row numbers (32 x int64), input rows, activation ping-pong, weights
  int lds_rows, lds_x, lds_act[2], lds_w;
  float threshold;
  long samp_n; unsigned long long samp_seed, samp_step; int samp_hb;
};

__global__ __launch_bounds__(256) void bcq_mask_kernel(const BcqMaskArgs a) {
  extern __shared__ __attribute__((aligned(16))) float bm_lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, kh = lane >> 5;
  const int row0 = blockIdx.x * QF_ROWS;
  const int L = a.n_lin - 1;
  float* wl = bm_lds + a.lds_w;
  float* X = bm_lds + a.lds_x;
  long* srow = reinterpret_cast<long*>(bm_lds + a.lds_rows);
  const int ldx = qf_r32(a.dims[0]) + 4;

  // layer 0's image is requested first: it is in flight while the row numbers and the rows themselves arrive
  float4 wr[QF_WREGS];
  qf_fetch_w(wr, a.params + a.w_off[0], a.dims[1], a.dims[0], t);
  asm volatile("" ::: "memory");
  if (t < QF_ROWS) {
    const int b = row0 + t;
    long r = 0L;
    if (b < a.B) r = a.samp_n > 0 ? (long)feistel_index(a.samp_n, b, a.samp_seed, a.samp_step, a.samp_hb) : (long)a.idx[b];
    srow[t] = r;
  }
  qf_barrier();
  QfInput xin;
  qf_input_rows(xin, ldx, nullptr, row0, a.B, t, QF_ROWS, srow);
  qf_input_load(xin, ldx, a.next_states, a.n_rs, row0, a.B, a.dims[0], t);      // rows past B, columns past S: zeros
  qf_input_store(xin, X, ldx, t);

  for (int l = 0; l <= L; ++l) {
    const int N = a.dims[l + 1], K = a.dims[l];
    qf_park_w(wl, wr, N, K, t);
    qf_barrier();                                   // input rows / layer l-1's output and this image are in LDS
    if (l < L) {
      qf_fetch_w(wr, a.params + a.w_off[l + 1], a.dims[l + 2], N, t);
      asm volatile("" ::: "memory");                // keep the requests in front of the MFMA loop
    }
    const float* in = l == 0 ? X : bm_lds + a.lds_act[(l - 1) & 1];
    float* out = bm_lds + a.lds_act[l & 1];
    const float* bl = wl + qf_r32(N) * (qf_rk(K) + 4);                           // bias row of the parked image
    qf_forward(in, qf_r32(K) + 4, wl, K, N, bl, l < L, out, qf_r32(N) + 4, wave, li, kh);
    qf_barrier();
  }

  // softmax + threshold: eight lanes per row; each forms the row's maximum and sum itself in softmax_mask_kernel's
  // order (same bits in all eight) and writes the actions sub, sub + 8, ...
  const int A = a.dims[L + 1], ldq = qf_r32(A) + 4;
  const int r = t >> 3, sub = t & 7;
  const int b = row0 + r;
  if (b < a.B) {
    const float* z = bm_lds + a.lds_act[L & 1] + r * ldq;
    float mx = -INFINITY;
    for (int j = 0; j < A; ++j) mx = fmaxf(mx, z[j]);
    float se = 0.f;
    for (int j = 0; j < A; ++j) se += expf(z[j] - mx);
    float* m = a.mask + (long)b * A;
    for (int j = sub; j < A; j += 8) {
      const float pj = expf(z[j] - mx) / se;
      m[j] = pj > a.threshold ? 1.f : 0.f;
    }
  }
}

// multi-launch fallback (a behaviour network the one-block plan does not cover): rows idx[b] of next_states -> the
// engine's zero-padded staging rows
__global__ __launch_bounds__(256) void bcq_gather_kernel(const float* __restrict__ next_states, long n_rs,
                                                         const int64_t* __restrict__ idx, float* __restrict__ xs, int B, int S,
                                                         int ld) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * ld) return;
  const int b = (int)(i / ld), c = (int)(i - (long)b * ld);
  xs[i] = c < S ? next_states[idx[b] * n_rs + c] : 0.f;
}

}  // namespace porl
