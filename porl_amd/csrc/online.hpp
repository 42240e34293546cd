// Online Q-learning: one-launch record and act kernels for the environment loop of the Q-learning trainers
// (porl_qnet_record / porl_qnet_act, include/porl_hip.h; src/porl/train/dqn_trainer.py:119-180).
//
//   online_record_kernel  one transition -> slot `slot` of the device replay mirror.  The transition travels in the
//                         kernel arguments (copied at launch), so the host never owns a buffer the device still reads.
//   online_act_kernel     greedy action(s) of 1..8 states: a GEMV chain over the engine's parameter images in ONE
//                         workgroup.  Weights stream from global memory straight into VGPRs (float4 per lane, each
//                         weight read once and never shared across waves, so an LDS round trip would be pure
//                         overhead); the B <= 8 activation rows live in LDS between layers.  Epilogue: argmax over
//                         the actions (lowest index on ties, NaN counts as the maximum, as torch.argmax), after the
//                         C51 expectation sum_i softmax(z)_i support_i or the QR quantile mean when asked.  The
//                         action(s) and a copy of the last step's loss statistics land in one record the host reads.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace porl {

constexpr int ONL_MAX_B = 8;           // states per act launch
constexpr int ONL_MAX_W = 1024;        // widest layer: 2 x 8 x 1024 fp32 activation rows = 64 KiB of LDS
constexpr int ONL_MAX_INLINE = 256;    // inline state floats (B x S) carried in the act kernel's arguments
constexpr int ONL_MAX_RECORD_S = 480;  // state width of a recorded transition: 2 x 480 floats + header < 4 KiB of arguments
constexpr int ONL_MAX_LIN = 9;         // PORL_MAX_HIDDEN + 1

struct OnlineRecordArgs {
  float* states;
  float* next_states;
  int64_t* actions;
  float* rewards;
  float* dones;
  int64_t slot;
  int64_t action;
  float reward, done;
  int S;
  float x[2 * ONL_MAX_RECORD_S];       // state | next_state
};

__global__ __launch_bounds__(256) void online_record_kernel(OnlineRecordArgs a) {
  const int64_t row = a.slot * a.S;
  for (int i = threadIdx.x; i < a.S; i += blockDim.x) {
    a.states[row + i] = a.x[i];
    a.next_states[row + i] = a.x[a.S + i];
  }
  if (threadIdx.x == 0) {
    a.actions[a.slot] = a.action;
    a.rewards[a.slot] = a.reward;
    a.dones[a.slot] = a.done;
  }
}

struct OnlineActArgs {
  const float* params;
  int64_t w_off[ONL_MAX_LIN], b_off[ONL_MAX_LIN];
  int wld[ONL_MAX_LIN];
  int dims[ONL_MAX_LIN + 1];
  int n_lin;
  int B;
  int ldx;                             // LDS row stride of the activation buffers (round4 of the widest layer)
  const float* states;                 // device rows (row stride s_rs), or NULL: x_inline
  int64_t s_rs;
  int kind;                            // 0 argmax of the outputs, 1 C51 expectation, 2 QR mean
  int n_act, n_sub;
  const float* support;                // C51: n_sub atoms
  const float* stats;                  // n_stats floats copied to the record (may be NULL)
  int n_stats;
  int32_t* out;                        // record: [0, 8) actions, [8, 11) fp32 statistics
  float x_inline[ONL_MAX_INLINE];
};

__device__ inline bool onl_better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;             // NaN beats every number
  if (vn || v == bv) return i < bi;
  return v > bv;
}

__global__ __launch_bounds__(256) void online_act_kernel(OnlineActArgs a) {
  extern __shared__ float onl_lds[];   // 2 x B x ldx
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = a.B, ldx = a.ldx;
  float* buf[2] = {onl_lds, onl_lds + B * ldx};
  const int S = a.dims[0];
  for (int i = tid; i < 2 * B * ldx; i += 256) {
    const int b = i / ldx, k = i - b * ldx;
    float v = 0.0f;
    if (b < B && k < S) v = a.states ? a.states[b * a.s_rs + k] : a.x_inline[b * S + k];
    onl_lds[i] = v;
  }
  __syncthreads();
  for (int l = 0; l < a.n_lin; ++l) {
    const int K = a.dims[l], Nn = a.dims[l + 1], K4 = (K + 3) >> 2;
    int G = 1;                         // lanes per output row: the smallest power of two covering K / 4 float4s
    while (G < K4 && G < 64) G <<= 1;
    const int rpw = 64 / G, gl = lane & (G - 1), sub = lane / G;
    const float* W = a.params + a.w_off[l];
    const float* bias = a.params + a.b_off[l];
    const float* in = buf[l & 1];
    float* out = buf[(l + 1) & 1];
    const bool relu = l + 1 < a.n_lin;
    for (int j0 = wave * rpw; j0 < Nn; j0 += 4 * rpw) {     // wave-uniform trip count: every lane reaches the shuffles
      const int j = j0 + sub;
      const bool valid = j < Nn;
      float acc[ONL_MAX_B];
#pragma unroll
      for (int b = 0; b < ONL_MAX_B; ++b) acc[b] = 0.0f;
      if (valid) {
        const float* wr = W + (int64_t)j * a.wld[l];
#pragma unroll 4
        for (int c = gl; c < K4; c += G) {
          const float4 w = *reinterpret_cast<const float4*>(wr + 4 * c);
#pragma unroll
          for (int b = 0; b < ONL_MAX_B; ++b) {
            if (b < B) {
              const float4 x = *reinterpret_cast<const float4*>(in + b * ldx + 4 * c);
              acc[b] += w.x * x.x + w.y * x.y + w.z * x.z + w.w * x.w;
            }
          }
        }
      }
      for (int off = G >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int b = 0; b < ONL_MAX_B; ++b) acc[b] += __shfl_xor(acc[b], off, 64);
      }
      if (valid && gl == 0) {
        const float bj = bias[j];
#pragma unroll
        for (int b = 0; b < ONL_MAX_B; ++b) {
          if (b < B) {
            float v = acc[b] + bj;
            out[b * ldx + j] = relu ? fmaxf(v, 0.0f) : v;
          }
        }
      }
    }
    // the next layer reads whole float4s: the columns up to round4(Nn) must be zero, not a wider layer's leftovers
    const int padw = ((Nn + 3) & ~3) - Nn;
    if (tid < B * padw) out[(tid / padw) * ldx + Nn + tid % padw] = 0.0f;
    __syncthreads();
  }
  const float* q = buf[a.n_lin & 1];
  float* val = buf[(a.n_lin + 1) & 1];
  const int A = a.n_act, NS = a.n_sub;
  for (int i = tid; i < B * A; i += 256) {
    const int b = i / A, act = i - b * A;
    const float* z = q + b * ldx + act * NS;
    float v;
    if (a.kind == 1) {
      float m = z[0];
      for (int k = 1; k < NS; ++k) m = fmaxf(m, z[k]);
      float se = 0.0f, sv = 0.0f;
      for (int k = 0; k < NS; ++k) {
        const float e = __expf(z[k] - m);
        se += e;
        sv += e * a.support[k];
      }
      v = sv / se;
    } else if (a.kind == 2) {
      float s = 0.0f;
      for (int k = 0; k < NS; ++k) s += z[k];
      v = s / (float)NS;
    } else {
      v = z[0];
    }
    val[b * ldx + act] = v;
  }
  __syncthreads();
  for (int b = wave; b < B; b += 4) {
    float bv = val[b * ldx];
    int bi = 0;
    for (int i = lane; i < A; i += 64) {
      const float v = val[b * ldx + i];
      if (onl_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (onl_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) a.out[b] = bi;
  }
  if (tid < a.n_stats) reinterpret_cast<float*>(a.out)[8 + tid] = a.stats[tid];
}

}  // namespace porl
