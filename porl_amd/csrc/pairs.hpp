// Staging of a goal-conditioned behaviour-cloning batch (reference agent/por.py:178, `concat([obs, next_obs], dim=1)`
// with the actions as regression target) straight into the IQL engine's staging buffers — no concatenated tensor, no
// staging copy:
//
//   xs[i] = [ src_s[0:S] | src_g[goal_col : goal_col + G] | 0 up to Sp ]        Sp = ru4(S + G)
//   xt[i] = [ action columns (A) | 0 up to Dp ]
//   w[i]  = 1.0f                     the per-row weight policy_nll_kernel reads through its `weight` argument
//
// One launch, one wave per batch row.  The three segments come from dense (or strided) tensors — row i of each — or from
// rows of a packed store [s | r | s' | d | a]: row `start` gives s and a, row `goal` the goal columns.  Which rows:
//   PAIR_DENSE      row i of every source
//   PAIR_GIVEN      start[i], goal[i] (goal == nullptr: the start row again; goal_col = S + 1 is then POR's [s | s'])
//   PAIR_HINDSIGHT  drawn here with the counter stream of ep_pairs_kernel (episodes.hpp): the same (seed, step) gives
//                   the pairs of porl_hindsight_pairs, index for index
//   PAIR_PERMUTED   `batch` distinct rows by feistel_index(seed, step) (kernels.hpp), goal row = start row
// A row number outside [0, n_rows) — a caller's index, or what a damaged episode table yields — is never read: the
// whole staged row becomes NaN (porl_gather_pairs' rule), and the loss says so.
//
// The s segment starts a row on both sides, so it moves as 16-byte lanes when the source pitch and base allow; the goal
// segment lands at column S (and leaves at goal_col), the actions leave at 2S + 2: those move float by float, as in
// ep_gather_pairs_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace porl {

enum PairMode { PAIR_DENSE = 0, PAIR_GIVEN = 1, PAIR_HINDSIGHT = 2, PAIR_PERMUTED = 3 };

// one segment's source: sample row r is the floats at base + r * stride + col
struct PairSrc { const float* base; long long stride; int col; };

struct PairStageArgs {
  PairSrc s, g, a;
  long long n_rows;                                   // rows every source holds (PAIR_DENSE: the batch)
  int mode;
  const long long* start; const long long* goal;      // PAIR_GIVEN (goal may be null)
  const long long* ep_starts; const long long* ep_lengths; long long E; uint64_t key;   // PAIR_HINDSIGHT
  uint64_t seed, step; int hb;                        // PAIR_PERMUTED
  int batch, S, G, A, Sp, Dp;
  float* xs; float* xt; float* w;
  long long* start_out; long long* goal_out;          // optional: the rows used
};

// ep_pairs_kernel's draw for sample i, statement for statement
__device__ __forceinline__ void pair_draw_hindsight(const PairStageArgs& a, int i, long long& s, long long& g) {
  const uint64_t c = 3ull * (uint64_t)i;
  const long long tr = (long long)__umul64hi(ep_sm64(a.key ^ ep_sm64(c)), (uint64_t)a.E);
  const double u1 = (double)(ep_sm64(a.key ^ ep_sm64(c + 1)) >> 11) * 0x1.0p-53;
  const double u2 = (double)(ep_sm64(a.key ^ ep_sm64(c + 2)) >> 11) * 0x1.0p-53;
  s = g = -1;
  if (tr >= 0 && tr < a.E) {
    const long long len = a.ep_lengths[tr], st = a.ep_starts[tr];
    const long long hi = len > 0 ? len - 1 : 0;
    const long long t1 = ep_time_index(u1, hi, hi), t2 = ep_time_index(u2, len, hi);
    s = st + (t1 < t2 ? t1 : t2);
    g = st + (t1 < t2 ? t2 : t1);
  }
}

__global__ __launch_bounds__(256) void stage_pairs_kernel(const PairStageArgs a) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= a.batch) return;                            // whole waves leave; no barrier below
  long long si = i, gi = i;
  if (a.mode == PAIR_GIVEN) { si = a.start[i]; gi = a.goal ? a.goal[i] : si; }
  else if (a.mode == PAIR_HINDSIGHT) pair_draw_hindsight(a, i, si, gi);
  else if (a.mode == PAIR_PERMUTED) si = gi = feistel_index(a.n_rows, i, a.seed, a.step, a.hb);
  const int S = a.S, G = a.G;
  float* xs = a.xs + (size_t)i * a.Sp;
  float* xt = a.xt + (size_t)i * a.Dp;
  if (lane == 0) {
    a.w[i] = 1.0f;
    if (a.start_out) a.start_out[i] = si;
    if (a.goal_out) a.goal_out[i] = gi;
  }
  if (si < 0 || si >= a.n_rows || gi < 0 || gi >= a.n_rows) {
    const float qnan = __int_as_float(0x7FC00000);
    for (int c = lane; c < a.Sp; c += 64) xs[c] = qnan;
    for (int c = lane; c < a.Dp; c += 64) xt[c] = qnan;
    return;
  }
  const float* __restrict__ ss = a.s.base + si * a.s.stride + a.s.col;
  const float* __restrict__ sg = a.g.base + gi * a.g.stride + a.g.col;
  const float* __restrict__ sa = a.a.base + si * a.a.stride + a.a.col;
  // staging rows start on 16-byte boundaries (Sp % 4 == 0, aligned workspace); the source decides
  const bool vec = a.s.col == 0 && (a.s.stride & 3) == 0 && (reinterpret_cast<uintptr_t>(a.s.base) & 15) == 0;
  const int S4 = vec ? S & ~3 : 0;
  for (int c = lane * 4; c < S4; c += 256) *reinterpret_cast<float4*>(xs + c) = *reinterpret_cast<const float4*>(ss + c);
  for (int c = S4 + lane; c < S; c += 64) xs[c] = ss[c];
  for (int c = lane; c < G; c += 64) xs[S + c] = sg[c];
  for (int c = S + G + lane; c < a.Sp; c += 64) xs[c] = 0.f;
  for (int c = lane; c < a.Dp; c += 64) xt[c] = c < a.A ? sa[c] : 0.f;
}

}  // namespace porl
