// Implicit Quantile Network pieces that are not plain Linear layers (gfx950 only).
//
// Reference: src/porl/net/iqn_network.py:35-91 (IQNNetwork.forward / get_quantile_embedding) and
// src/porl/train/iqn_trainer.py:92-134 (IQNTrainer.learn).  The Linear layers of the network run on the grouped fp32-MFMA
// GEMM (gemm_f32.hpp) and the quantile-Huber head on iqn_loss_kernel (dist_losses.hpp); what is here is the HBM-bound glue
// between them, each a single pass over its tensor with 16-byte accesses where the rows allow it:
//   * cosine features cos(pi * i * tau), i = 1..E                                     (iqn_network.py:74-91)
//   * the Hadamard product of state features (B, H) with quantile embeddings (B*N, H)   (iqn_network.py:58-62) + backward
//   * gather / scatter of the taken action's quantile values along the action axis     (iqn_trainer.py:101-103)
//   * Double-DQN action choice on the tau-mean of the online net + Bellman targets     (iqn_trainer.py:108-121)
//   * torch.nn.utils.clip_grad_norm_ on a flat gradient buffer                         (iqn_trainer.py:131)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace porl {

// out[r, i] = cos(pi * (i + 1) * taus[r]) in the reference's fp32 operation order: (fl32(pi) * idx) * tau, then cos
__global__ __launch_bounds__(256) void iqn_cos_embed_kernel(const float* __restrict__ taus, long n, int E,
                                                            float* __restrict__ out) {
  const long total = n * E;
  const float pi = 3.14159265358979323846f;
  for (long f = (long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long)gridDim.x * 256) {
    const long r = f / E;
    const int i = (int)(f - r * E);
    out[f] = cosf(__fmul_rn(__fmul_rn(pi, (float)(i + 1)), taus[r]));
  }
}

// out[(b*N + n), :] = feat[b, :] * emb[(b*N + n), :]
__global__ __launch_bounds__(256) void iqn_hadamard_kernel(const float* __restrict__ feat, long ldf,
                                                           const float* __restrict__ emb, int batch, int n_tau, int H,
                                                           float* __restrict__ out, int aligned16) {
  const long rows = (long)batch * n_tau;
  if (aligned16 && (H & 3) == 0 && (ldf & 3) == 0) {
    const int H4 = H >> 2;
    const long total = rows * H4;
    for (long f = (long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long)gridDim.x * 256) {
      const long r = f / H4;
      const int c = (int)(f - r * H4);
      const long b = r / n_tau;
      const float4 s = *reinterpret_cast<const float4*>(feat + b * ldf + 4 * c);
      const float4 e = *reinterpret_cast<const float4*>(emb + r * H + 4 * c);
      *reinterpret_cast<float4*>(out + r * H + 4 * c) = make_float4(s.x * e.x, s.y * e.y, s.z * e.z, s.w * e.w);
    }
  } else {
    const long total = rows * H;
    for (long f = (long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long)gridDim.x * 256) {
      const long r = f / H;
      const int c = (int)(f - r * H);
      out[f] = feat[(r / n_tau) * ldf + c] * emb[f];
    }
  }
}

// demb[(b*N + n), :] = dout[(b*N + n), :] * feat[b, :];   dfeat[b, :] = sum_n dout[(b*N + n), :] * emb[(b*N + n), :]
// (n ascending: the order of torch's sum over the expanded dimension is not specified; fp32, sequential).
// One thread per (b, column); either output may be null.
__global__ __launch_bounds__(256) void iqn_hadamard_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ feat,
                                                               long ldf, const float* __restrict__ emb, int batch, int n_tau,
                                                               int H, float* __restrict__ dfeat, float* __restrict__ demb) {
  const long total = (long)batch * H;
  for (long f = (long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long)gridDim.x * 256) {
    const long b = f / H;
    const int c = (int)(f - b * H);
    const float s = feat[b * ldf + c];
    float acc = 0.f;
    for (int n = 0; n < n_tau; ++n) {
      const long o = (b * n_tau + n) * H + c;
      const float d = dout[o];
      if (dfeat) acc = fmaf(d, emb[o], acc);
      if (demb) demb[o] = d * s;
    }
    if (dfeat) dfeat[f] = acc;
  }
}

// out[b, n] = z[b, n, actions[b]]   (an action outside 0..A-1 gives NaN: the reference's gather raises there)
__global__ __launch_bounds__(256) void iqn_select_kernel(const float* __restrict__ z, const int64_t* __restrict__ actions,
                                                         int batch, int n_tau, int A, float* __restrict__ out) {
  const long total = (long)batch * n_tau;
  for (long f = (long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long)gridDim.x * 256) {
    const int64_t a = actions[f / n_tau];
    out[f] = (a >= 0 && a < A) ? z[f * A + a] : __builtin_nanf("");
  }
}

// dz[b, n, a] = (a == actions[b]) ? dsel[b, n] : 0
__global__ __launch_bounds__(256) void iqn_scatter_kernel(const float* __restrict__ dsel, const int64_t* __restrict__ actions,
                                                          int batch, int n_tau, int A, float* __restrict__ dz) {
  const long total = (long)batch * n_tau * A;
  for (long f = (long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long)gridDim.x * 256) {
    const long r = f / A;
    const int a = (int)(f - r * A);
    dz[f] = (int64_t)a == actions[r / n_tau] ? dsel[r] : 0.f;
  }
}

// Per sample b: a* = argmax_a mean_n z_online[b, n, a] (first maximum, like torch.argmax; the mean is the fp32 sum over n
// ascending divided by N), td[b, n] = r[b] + gamma * z_target[b, n, a*] * (1 - done[b])        (iqn_trainer.py:108-121)
__global__ __launch_bounds__(256) void iqn_target_kernel(const float* __restrict__ z_online, const float* __restrict__ z_target,
                                                         const float* __restrict__ rewards, const float* __restrict__ dones,
                                                         float gamma, int batch, int n_tau, int A, float* __restrict__ td,
                                                         int64_t* __restrict__ next_actions) {
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < batch; b += (long)gridDim.x * 256) {
    int best = 0;
    float best_q = 0.f;
    for (int a = 0; a < A; ++a) {
      float s = 0.f;
      for (int n = 0; n < n_tau; ++n) s += z_online[(b * n_tau + n) * A + a];
      const float q = s / (float)n_tau;
      if (a == 0 || q > best_q) { best = a; best_q = q; }
    }
    if (next_actions) next_actions[b] = best;
    const float r = rewards[b], nd = 1.f - dones[b];
    for (int n = 0; n < n_tau; ++n)
      td[b * n_tau + n] = __fadd_rn(r, __fmul_rn(__fmul_rn(gamma, z_target[(b * n_tau + n) * A + best]), nd));
  }
}

// ---- clip_grad_norm_ --------------------------------------------------------------------------------------------------
// total = sqrt(sum g^2) (fp64 partial sums per block in a fixed order, one block adds the partials), coefficient
// min(1, max_norm / (total + 1e-6)) as torch forms it in fp32, applied in a second pass.
constexpr int CLIP_BLOCKS = 256;
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, long n, double* __restrict__ partial) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const double v = (double)g[i];
    s += v * v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void clip_coef_kernel(const double* __restrict__ partial, int nblocks, float max_norm,
                                                        float* __restrict__ norm_coef) {
  __shared__ double red[256];
  red[threadIdx.x] = (int)threadIdx.x < nblocks ? partial[threadIdx.x] : 0.0;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = (float)sqrt(red[0]);
    const float coef = max_norm / (total + 1e-6f);
    norm_coef[0] = total;
    norm_coef[1] = coef < 1.f ? coef : 1.f;
  }
}
__global__ __launch_bounds__(256) void scale_by_kernel(float* __restrict__ g, long n, const float* __restrict__ norm_coef) {
  const float c = norm_coef[1];
  if (c == 1.f) return;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) g[i] *= c;
}


// =====================================================================================================================
// One-call learn step / native act of the IQN engine (porl_iqn_learn / porl_iqn_act, csrc/iqn_api.inc): the glue above
// fused so that a step runs from a handful of launches with no intermediate tensor between them.
// =====================================================================================================================
constexpr int IQN_MAX_E = 128;        // cosine features: one (64 columns x E) weight panel + 32 feature rows in 49 KiB of LDS
constexpr int IQN_MAX_TAU = 256;      // fractions per state (N', N'', N_policy): one wave's Bellman targets in LDS
constexpr int IQN_MAX_A = 64;         // actions: one lane per action in the Double-DQN choice
constexpr int IQN_MIX_ROWS = 32, IQN_MIX_COLS = 64;

// out[(b, n), :] = feat[b, :] * (cos_features(tau[b, n]) . We^T + be) for up to three problems per launch
// (iqn_network.py:52-62: quantile_embedding(get_quantile_embedding(tau)) times the state features).  The cosine features
// are generated while the operand is staged (iqn_cos_embed_kernel's expression) and never written; the product is one
// fmaf chain from zero in the k order of gemm_f32_kernel — within each group of eight k: 0, 4, 1, 5, 2, 6, 3, 7, because
// its v_mfma_f32_32x32x2_f32 takes k = 8g + j from lanes 0-31 and k = 8g + 4 + j from lanes 32-63 and adds them in that
// order — then + bias, then * feat, so the result has the bits of porl_iqn_cos_embed -> porl_gemm_f32(bias) ->
// porl_iqn_hadamard.  emb (optional): the un-multiplied embedding rows, kept for the backward of the problem that has one.
struct IqnMixProb {
  const float* feat; long ldf;      // (batch, H) state features
  const float* taus;                // (batch * n_tau)
  const float* We; long ldw;        // (H, E)
  const float* be;                  // (H)
  float* out; long ldo;             // (batch * n_tau, H)
  float* emb;                       // (batch * n_tau, H) with row stride ldo, or null
  int rows, n_tau;
};
struct IqnMixArgs { IqnMixProb p[3]; int nprob, E, H; };

__global__ __launch_bounds__(256) void iqn_mix_kernel(const IqnMixArgs a) {
  __shared__ float Ws[IQN_MAX_E][IQN_MIX_COLS + 1];
  __shared__ float Cs[IQN_MIX_ROWS][IQN_MAX_E];
  const IqnMixProb& P = a.p[blockIdx.z];
  const int r0 = blockIdx.y * IQN_MIX_ROWS, c0 = blockIdx.x * IQN_MIX_COLS;
  if (r0 >= P.rows) return;
  const int tid = threadIdx.x, E = a.E;
  const float pi = 3.14159265358979323846f;
  for (int i = tid; i < IQN_MIX_COLS * E; i += 256) {
    const int c = i / E, k = i - c * E;
    Ws[k][c] = c0 + c < a.H ? P.We[(long)(c0 + c) * P.ldw + k] : 0.f;
  }
  for (int i = tid; i < IQN_MIX_ROWS * E; i += 256) {
    const int r = i / E, k = i - r * E;
    Cs[r][k] = r0 + r < P.rows ? cosf(__fmul_rn(__fmul_rn(pi, (float)(k + 1)), P.taus[r0 + r])) : 0.f;
  }
  __syncthreads();
  const int c = tid & 63, rg = tid >> 6;           // a wave owns 8 rows: its feature reads are LDS broadcasts
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int k8 = 0; k8 < E; k8 += 8) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int k = k8 + (t >> 1) + 4 * (t & 1);    // 0, 4, 1, 5, 2, 6, 3, 7: the two lane halves of each MFMA
      if (k < E) {
        const float w = Ws[k][c];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(Cs[rg * 8 + j][k], w, acc[j]);
      }
    }
  }
  const int col = c0 + c;
  if (col >= a.H) return;
  const float bias = P.be[col];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int r = r0 + rg * 8 + j;
    if (r < P.rows) {
      const float e = __fadd_rn(acc[j], bias);
      if (P.emb) P.emb[(long)r * P.ldo + col] = e;
      P.out[(long)r * P.ldo + col] = __fmul_rn(P.feat[(long)(r / P.n_tau) * P.ldf + col], e);
    }
  }
}

// The loss head of IQNTrainer.learn (iqn_trainer.py:101-134) on the three networks' outputs, one wave per minibatch row:
// Double-DQN choice on the tau''-mean of the online net (iqn_target_kernel's sum order and first-maximum rule), Bellman
// targets, the taken action's quantiles (iqn_select_kernel), the pairwise quantile-Huber loss (iqn_loss_kernel's loop,
// statement for statement: same bits) and dL/dz scattered into the (B * N', ld) rows the backward chain reads, zero off
// the taken action and in the padding columns.  An action outside 0..A-1: zero gradient rows and a NaN row loss.
struct IqnHeadArgs {
  const float* z_cur;               // (B * Np, ld)  online net on s, tau'
  const float* z_on;                // (B * Npp, ld) online net on s', tau''
  const float* z_tg;                // (B * Npp, ld) target net on s', tau''
  long ld;
  const int64_t* actions; const float* rew; const float* done; const float* taus;    // taus: (B, Np)
  float* dz;                        // (B * Np, ld)
  float* row_loss;                  // (B)
  int64_t* next_actions;            // (B) or null
  int B, Np, Npp, A;
  float gamma, kappa, inv_batch;
};

__global__ __launch_bounds__(256) void iqn_head_kernel(const IqnHeadArgs a) {
  __shared__ float sh_t[4][IQN_MAX_TAU];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * 4 + wave;
  if (b >= a.B) return;
  const int A = a.A, Np = a.Np, Npp = a.Npp;
  // lane `act` sums its action's column over the fractions, n ascending; every lane then walks the A means in order
  float q = 0.f;
  if (lane < A) {
    float s = 0.f;
    for (int n = 0; n < Npp; ++n) s += a.z_on[(b * Npp + n) * a.ld + lane];
    q = s / (float)Npp;
  }
  int best = 0;
  float best_q = 0.f;
  for (int act = 0; act < A; ++act) {
    const float v = __shfl(q, act, 64);
    if (act == 0 || v > best_q) { best = act; best_q = v; }
  }
  if (a.next_actions && lane == 0) a.next_actions[b] = best;
  const float r = a.rew[b], nd = 1.f - a.done[b];
  float* T = sh_t[wave];
  for (int n = lane; n < Npp; n += 64)
    T[n] = __fadd_rn(r, __fmul_rn(__fmul_rn(a.gamma, a.z_tg[(b * Npp + n) * a.ld + best]), nd));
  __builtin_amdgcn_wave_barrier();
  const int64_t at64 = a.actions[b];
  const bool ok = at64 >= 0 && at64 < A;
  const int at = ok ? (int)at64 : 0;
  float loss = 0.f;
  for (int i = lane; i < Np; i += 64) {
    float* drow = a.dz + (b * Np + i) * a.ld;
    float d = 0.f;
    if (ok) {
      const float th = a.z_cur[(b * Np + i) * a.ld + at], tau = a.taus[b * Np + i];
      float g = 0.f;
      for (int j = 0; j < Npp; ++j) {
        const float u = T[j] - th, au = fabsf(u);
        const float w = fabsf(tau - (u < 0.f ? 1.f : 0.f));
        const bool quad = au <= a.kappa;
        loss += w * (quad ? 0.5f * u * u : a.kappa * (au - 0.5f * a.kappa));
        g += w * (quad ? u : (u > 0.f ? a.kappa : -a.kappa));
      }
      d = -g * a.inv_batch / ((float)Np * (float)Npp);
    }
    for (int c = 0; c < (int)a.ld; ++c) drow[c] = (ok && c == at) ? d : 0.f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) loss += __shfl_xor(loss, o);
  if (lane == 0) a.row_loss[b] = ok ? loss / ((float)Np * (float)Npp) : __builtin_nanf("");
}

// iqn_hadamard_bwd_kernel with the ReLU mask of the feature net's output folded in (the chain feat = relu(...) ends in):
// dfeat[b, c] = 1[feat[b, c] > 0] * sum_n dout[(b, n), c] * emb[(b, n), c] (n ascending), demb = dout * feat.
__global__ __launch_bounds__(256) void iqn_hadamard_bwd_relu_kernel(const float* __restrict__ dout, const float* __restrict__ feat,
                                                                    const float* __restrict__ emb, int batch, int n_tau, int H,
                                                                    long ld, float* __restrict__ dfeat, float* __restrict__ demb) {
  const long total = (long)batch * H;
  for (long f = (long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long)gridDim.x * 256) {
    const long b = f / H;
    const int c = (int)(f - b * H);
    const float s = feat[b * ld + c];
    float acc = 0.f;
    for (int n = 0; n < n_tau; ++n) {
      const long o = (b * n_tau + n) * ld + c;
      const float d = dout[o];
      acc = fmaf(d, emb[o], acc);
      demb[o] = d * s;
    }
    dfeat[b * ld + c] = s > 0.f ? acc : 0.f;
  }
}

// Gradient of the quantile-embedding Linear without its input tensor: dW[h, k] = sum_r demb[r, h] * cos(pi (k+1) tau[r]),
// db[h] = sum_r demb[r, h], r ascending in one fp32 chain each.  Block (x, y): 16 columns h x 16 features k, one (h, k)
// pair per thread; the gradient rows and the cosine features of 128 rows at a time are staged / generated in LDS.
constexpr int IQN_WG_T = 16, IQN_WG_ROWS = 128;
__global__ __launch_bounds__(256) void iqn_embed_wgrad_kernel(const float* __restrict__ demb, long ld, const float* __restrict__ taus,
                                                              int rows, int H, int E, float* __restrict__ dW, long ldw,
                                                              float* __restrict__ db) {
  __shared__ float Ds[IQN_WG_ROWS][IQN_WG_T + 1];
  __shared__ float Cs[IQN_WG_ROWS][IQN_WG_T + 1];
  const int tid = threadIdx.x, c = tid & (IQN_WG_T - 1), kk = tid / IQN_WG_T;
  const int c0 = blockIdx.x * IQN_WG_T, k0 = blockIdx.y * IQN_WG_T;
  const float pi = 3.14159265358979323846f;
  float acc = 0.f, accb = 0.f;
  for (int r0 = 0; r0 < rows; r0 += IQN_WG_ROWS) {
    __syncthreads();
    for (int i = tid; i < IQN_WG_ROWS * IQN_WG_T; i += 256) {
      const int r = i / IQN_WG_T, j = i - r * IQN_WG_T;
      const bool in = r0 + r < rows;
      Ds[r][j] = (in && c0 + j < H) ? demb[(long)(r0 + r) * ld + c0 + j] : 0.f;
      Cs[r][j] = (in && k0 + j < E) ? cosf(__fmul_rn(__fmul_rn(pi, (float)(k0 + j + 1)), taus[r0 + r])) : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < IQN_WG_ROWS; ++r) {
      const float d = Ds[r][c];
      acc = fmaf(d, Cs[r][kk], acc);
      accb += d;
    }
  }
  if (c0 + c >= H) return;
  if (k0 + kk < E) dW[(long)(c0 + c) * ldw + k0 + kk] = acc;
  if (blockIdx.y == 0 && kk == 0) db[c0 + c] = accb;
}

// First feature layer of the act path on ONE state: out[h] = relu(W[h, :] . x + b[h]).  The state is a row of a device
// array or travels in the kernel's arguments (right after env.reset() no device row holds it).
constexpr int IQN_ACT_MAX_INLINE = 256;
struct IqnActL0Args {
  const float* W; long ldw; const float* bias; float* out;
  const float* state;               // device row, or null: x_inline
  int S, H;
  float x_inline[IQN_ACT_MAX_INLINE];
};
__global__ __launch_bounds__(256) void iqn_act_l0_kernel(const IqnActL0Args a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int h = blockIdx.x * 4 + wave;              // one wave per output: coalesced weight rows
  if (h >= a.H) return;
  float s = 0.f;
  for (int k = lane; k < a.S; k += 64) s = fmaf(a.W[(long)h * a.ldw + k], a.state ? a.state[k] : a.x_inline[k], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) a.out[h] = fmaxf(s + a.bias[h], 0.f);
}

// Last value layer (H -> A) on the n_tau rows of one state, the mean over the fractions (fp32 sum, n ascending, / N), the
// first-maximum argmax (NaN counts as the maximum, as torch.argmax) and the action into a record laid out like
// porl_qnet_act's: int32 action at word 0, fp32 copies of stats[0, n_stats) from word 8.  One workgroup.
struct IqnActHeadArgs {
  const float* hv; long ld;         // (n_tau, H) hidden rows of the value net
  const float* W; long ldw; const float* bias;      // (A, H), (A)
  const float* stats; int n_stats;
  int32_t* out;
  int n_tau, H, A;
  int vec;                          // rows of hv and W may be read 16 bytes at a time
};
__global__ __launch_bounds__(1024) void iqn_act_head_kernel(const IqnActHeadArgs a) {
  extern __shared__ float iqn_z[];                  // (n_tau, A)
  __shared__ float qs[IQN_MAX_A];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
  for (int n = wave; n < a.n_tau; n += nwaves) {    // a wave per row: the row is read once per four actions
    const float* x = a.hv + (long)n * a.ld;
    for (int a0 = 0; a0 < a.A; a0 += 4) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.vec) {
        for (int k4 = lane; k4 < (a.H >> 2); k4 += 64) {
          const float4 xv = *reinterpret_cast<const float4*>(x + 4 * k4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (a0 + j < a.A) {
              const float4 w = *reinterpret_cast<const float4*>(a.W + (long)(a0 + j) * a.ldw + 4 * k4);
              acc[j] = fmaf(xv.x, w.x, fmaf(xv.y, w.y, fmaf(xv.z, w.z, fmaf(xv.w, w.w, acc[j]))));
            }
          }
        }
      } else {
        for (int k = lane; k < a.H; k += 64) {
          const float xv = x[k];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (a0 + j < a.A) acc[j] = fmaf(xv, a.W[(long)(a0 + j) * a.ldw + k], acc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off);
        if (lane == 0 && a0 + j < a.A) iqn_z[n * a.A + a0 + j] = acc[j] + a.bias[a0 + j];
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < a.A) {
    float s = 0.f;
    for (int n = 0; n < a.n_tau; ++n) s += iqn_z[n * a.A + threadIdx.x];
    qs[threadIdx.x] = s / (float)a.n_tau;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = 0;
    float bv = qs[0];
    for (int i = 1; i < a.A; ++i) {
      const float v = qs[i];
      if (bv == bv && (v != v || v > bv)) { best = i; bv = v; }
    }
    a.out[0] = best;
  }
  if ((int)threadIdx.x < a.n_stats) reinterpret_cast<float*>(a.out)[8 + threadIdx.x] = a.stats[threadIdx.x];
}

}  // namespace porl
