// IQN for a loop that moves N robots per launch and never returns to the host (porl_iqn_draw_taus, porl_iqn_select_rows,
// porl_iqn_act_rows, porl_iqn_learn_sampled, include/porl_hip.h; train/vector_iqn.py): the fractions tau, tau', tau'' drawn on
// the device from a keyed counter stream, the staging of one chunk of robots, and the head that turns a chunk's quantile
// values into one epsilon-greedy action per robot.  The Linear layers stay on the grouped GEMM and the cosine features on
// iqn_mix_kernel (iqn.hpp), so the (m * K, ld) values z the head reads have the bits of the learn step's forward.
//
// The fraction stream.  Element e of draw `draw` of use `use` under `seed`:
//     key     = sm64(seed ^ IQN_TAU_TAG ^ use)                use: 0 acting, 1 tau', 2 tau''
//     counter = (draw << 32) | e                               draw < 2^32, e < 2^32 (the host checks both ranges)
//     tau     = (float)(sm64(key ^ sm64(counter)) >> 40) * 2^-24
// sm64 is ep_sm64 (episodes.hpp, splitmix64's finaliser after its increment).  The top 24 bits of a 64-bit word convert to
// fp32 exactly, so every value is a multiple of 2^-24 in [0, 1) — 1.0 cannot occur — the form of torch.rand's fp32 draws.
// sm64 is a bijection: two uses (different keys) never give the same word at one counter, and two counters never the same
// word under one key.  IQN_TAU_TAG = sm64(0x49514E5441554652), the ASCII bytes "IQNTAUFR": the exploration and reset
// streams key by sm64(seed ^ sm64(robot)), the prioritized sampler by sm64(seed ^ PER_KEY_TAG) (per_vector.hpp).
// Element numbering:
//     acting    e = (env_offset + i) * n_tau + j   robot i of the call, fraction j; draw = the act-step t.  A robot's
//               fractions do not depend on chunking, grid shape, or how robots are split over simulators;
//     learning  e = b * n + j                      minibatch row b, fraction j of n; draw = the learn-draw counter.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "episodes.hpp"          // ep_sm64
#include "iqn.hpp"               // IQN_MAX_TAU, IQN_MAX_A
#include "navsim_discrete.hpp"   // nav_u01, NAV_EXACT: the exploration draws of qnet_select_kernel

namespace porl {

constexpr uint64_t IQN_TAU_TAG = 0x30C9E7BC03E23535ull;
constexpr int64_t IQN_TAU_MAX_DRAW = (int64_t(1) << 32) - 1;     // draw rides in the high 32 bits of the counter
constexpr int64_t IQN_TAU_MAX_ELEMS = int64_t(1) << 32;          // e in the low 32

__host__ __device__ __forceinline__ uint64_t iqn_tau_key(uint64_t seed, int use) {
  return ep_sm64(seed ^ IQN_TAU_TAG ^ (uint64_t)use);
}

__host__ __device__ __forceinline__ float iqn_tau(uint64_t key, uint64_t draw, uint64_t e) {
  return (float)(ep_sm64(key ^ ep_sm64((draw << 32) | e)) >> 40) * 0x1.0p-24f;
}

// Elements [first, first + count) of up to two streams, one thread per element (blockIdx.y: the job).  `out` is the
// caller's and may sit on any 4-byte boundary: scalar stores, coalesced.
struct IqnTauJob { float* out; uint64_t key, draw; int64_t first, count; };
struct IqnTauArgs { IqnTauJob job[2]; };

__global__ __launch_bounds__(256) void iqn_taus_kernel(const IqnTauArgs a) {
  const IqnTauJob& j = a.job[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < j.count) j.out[i] = iqn_tau(j.key, j.draw, (uint64_t)(j.first + i));
}

// Staging of one chunk of robots, rows [0, m) of `states` (the caller has advanced the pointers to the chunk):
//   * the states, row stride s_rs >= S, into rows of stride Sp = ru4(S) with the padding columns written as zero;
//   * the chunk's m * K fractions into `taus_out`: elements first_e .. first_e + m * K - 1 of the acting stream at draw
//     t, or a copy of the caller's `taus`.
// Thread f handles the f-th group of four floats of each job.  Both destinations are 16-byte aligned workspace regions of
// a multiple of four floats: every store is a float4.  A source group is read as one float4 when its address allows it
// and it lies inside the row / the array, float by float otherwise (a row of 362 floats starts on a 16-byte boundary
// only every other row).
struct IqnStageArgs {
  const float* states; long long s_rs;
  float* xs;                              // (m, Sp)
  const float* taus;                      // (m * K) or null: the stream
  float* taus_out;                        // ru4(m * K) floats
  uint64_t key, t;
  long long first_e;
  int m, S, Sp, K;
};

__global__ __launch_bounds__(256) void iqn_act_stage_kernel(const IqnStageArgs a) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  const int Sp4 = a.Sp >> 2;
  if (f < (long long)a.m * Sp4) {
    const int r = (int)(f / Sp4), c = 4 * (int)(f - (long long)r * Sp4);
    const float* src = a.states + r * a.s_rs + c;
    float4 v;
    if (c + 3 < a.S && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      v = *reinterpret_cast<const float4*>(src);
    } else {
      v.x = c < a.S ? src[0] : 0.f; v.y = c + 1 < a.S ? src[1] : 0.f;
      v.z = c + 2 < a.S ? src[2] : 0.f; v.w = c + 3 < a.S ? src[3] : 0.f;
    }
    *reinterpret_cast<float4*>(a.xs + (long long)r * a.Sp + c) = v;
  }
  const long long total = (long long)a.m * a.K, e = 4 * f;
  if (e < total) {
    float4 v;
    if (a.taus) {
      const float* src = a.taus + e;
      if (e + 3 < total && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        v = *reinterpret_cast<const float4*>(src);
      } else {
        v.x = src[0]; v.y = e + 1 < total ? src[1] : 0.f;
        v.z = e + 2 < total ? src[2] : 0.f; v.w = e + 3 < total ? src[3] : 0.f;
      }
    } else {
      const uint64_t e0 = (uint64_t)(a.first_e + e);
      v.x = iqn_tau(a.key, a.t, e0); v.y = e + 1 < total ? iqn_tau(a.key, a.t, e0 + 1) : 0.f;
      v.z = e + 2 < total ? iqn_tau(a.key, a.t, e0 + 2) : 0.f; v.w = e + 3 < total ? iqn_tau(a.key, a.t, e0 + 3) : 0.f;
    }
    *reinterpret_cast<float4*>(a.taus_out + e) = v;
  }
}

// The head of acting for rows of robots: z (n * K, ld) holds robot i's K quantile rows one after the other, A values each.
//   q[i, a] = (sum over n ascending of z[(i * K + n) * ld + a]) / (float)K      s = 0; s += ...; one fp32 chain per action
// — iqn_head_kernel's statement for the next state's action ranking, so acting and bootstrapping rank actions by the same
// bits — then qnet_select_kernel's rule as dist_select_kernel applies it: key sm64(seed ^ sm64(env_offset + i)), draws 0 and
// 1 of act-step t, u1 < epsilon explores with min(floor(A * u2), A - 1), otherwise arg-max with ties to the lowest index
// and the first NaN winning.  Values and action are written for every robot, also one that explores.
//
// Shape: ONE WAVE PER ROBOT, four robots per 256-thread block, no block barrier.  A robot's K * ld floats are contiguous:
// the wave copies them into its own 4 KiB of LDS in pieces of whole rows — lane-strided float4 loads when z and ld allow
// it, lane-strided floats otherwise, both coalesced, nothing read past the last value of the robot's last row — and lane
// a < A then adds column a of the piece, rows ascending: consecutive lanes read consecutive LDS words, so no bank is asked
// twice.  ld <= IQN_ROWS_MAX_LD keeps a row inside the piece.
constexpr int IQN_ROWS_LDS = 1024;          // floats per wave
constexpr int IQN_ROWS_MAX_LD = 128;

struct IqnRowsHeadArgs {
  const float* z; long long ld;          // (n * K, ld)
  float* q; long long q_rs;              // (n, >= A) action values out
  long long* out;                        // (n) actions out
  long long n, env_offset, t;
  double epsilon;
  uint64_t seed;
  int K, A;
  int vec;                               // z is 16-byte aligned and ld a multiple of 4
};

__global__ void __launch_bounds__(256)
iqn_rows_head_kernel(const IqnRowsHeadArgs a) {
  NAV_EXACT
  __shared__ float4 stage4[4][IQN_ROWS_LDS / 4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + wave;
  if (i >= a.n) return;                               // uniform over the wave; the kernel has no block barrier
  const int K = a.K, A = a.A, ld = (int)a.ld;
  float* L = reinterpret_cast<float*>(stage4[wave]);
  const float* __restrict__ zr = a.z + i * K * a.ld;
  const int piece = IQN_ROWS_LDS / ld;                // rows per piece, >= 8
  float s = 0.f;
  for (int n0 = 0; n0 < K; n0 += piece) {
    const int rows = K - n0 < piece ? K - n0 : piece;
    const int count = (rows - 1) * ld + A;            // up to the last value of the piece's last row
    const float* __restrict__ src = zr + (long long)n0 * ld;
    if (a.vec) {
      for (int k = lane; k < (count >> 2); k += 64) stage4[wave][k] = reinterpret_cast<const float4*>(src)[k];
      for (int k = (count & ~3) + lane; k < count; k += 64) L[k] = src[k];
    } else {
      for (int k = lane; k < count; k += 64) L[k] = src[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < A) {                                     // eight LDS reads in flight, then added in row order
      int n = 0;
      for (; n + 8 <= rows; n += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = L[(n + j) * ld + lane];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
      }
      for (; n < rows; ++n) s += L[n * ld + lane];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                  // the next piece overwrites what was just read
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  const float val = s / (float)K;
  if (lane < A) a.q[i * a.q_rs + lane] = val;
  // qnet_select_kernel's arg-max: ties to the lowest index, a NaN counts as the maximum, the first NaN wins
  float best = 0.f;
  long long pick = 0;
  for (int act = 0; act < A; ++act) {
    const float v = __shfl(val, act, 64);
    if (act == 0) best = v;
    else if (best == best && (v > best || v != v)) { best = v; pick = act; }
  }
  if (lane == 0) {
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
