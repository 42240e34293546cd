// Column statistics and the affine column pass of a resident row store — what `--normalize` needs from a dataset
// (por_train.py:141): mean / std of the observation columns, obs = (obs - mean) / std (util/util.py:146,160,177) and the
// reward rescaling r /= (max_ret - min_ret); r *= max_episode_steps that return_range (util/util.py:67-80) exists for.
//
// Statistics.  Per column the pass returns (mean, M2 = sum (x - mean)^2, min, max) in fp64.  Every accumulation is fp64
// and every combination of two partial results (n_a, mean_a, M2_a), (n_b, mean_b, M2_b) is the pairwise update
//     d = mean_b - mean_a,  n = n_a + n_b,  mean = mean_a + d * n_b / n,  M2 = M2_a + M2_b + d^2 * n_a * n_b / n
// so nothing ever forms sum x^2 (a column around 4096 with a spread of 2^-6 loses every bit of its variance that way),
// and a constant column has d = 0 at every level: M2 == 0.0 exactly.  min / max keep a NaN once they have seen one
// (numpy's min / max); the mean and M2 turn NaN by arithmetic.
//
// One refinement keeps the update honest for such a column.  A partial mean is a ROUNDED double m: the true mean is
// m + rho / n with a residual rho = sum (x - m) of the size of the rounding, and a d taken between two rounded means
// carries that error into d^2 n_a n_b / n in FIRST order — 2 d (n_a n_b / n) * ulp(4096) is several times the whole
// variance budget of a 1000-row column whose mean is 4e5 standard deviations from zero.  So a partial carries rho beside
// m, and M2 is kept about the stored m.  With c = m_a + d n_b / n the new centre, e_a = m_a - c, e_b = m_b - c (exact
// differences of neighbours):
//     rho = (n_a e_a + n_b e_b) + rho_a + rho_b
//     M2  = M2_a + M2_b + (n_a e_a^2 + n_b e_b^2) + 2 (e_a rho_a + e_b rho_b)
// which is the update above (n_a e_a^2 + n_b e_b^2 = d^2 n_a n_b / n) with the residual carried instead of dropped; a
// batch's own residual is one fma.  The last merge returns mean = m + rho / n and M2 - rho^2 / n.
//
// Launch structure (episodes.hpp): no floating-point atomics, no block ever waits for another block.
//   cs_tile_kernel     a block reduces CS_TILE consecutive rows x one chunk of <= CS_CHUNK columns to one partial per
//                      column and stores it; grid = (tiles, column chunks)
//   cs_merge_kernel    one thread per (group of CS_SWEEP consecutive partials, column) folds the group left to right;
//                      launched once per level until one partial is left, which it writes to `out`
// Row counts are never stored: partial i of level l covers rows [i * CS_TILE * CS_SWEEP^l, ...) cut at n_rows.  The
// order of every combination therefore follows from n_rows, n_cols and the constants below — not from the row pitch,
// the base address or which load path ran — and two calls on equal values return equal bits.
//
// Inside a tile.  With G = ceil(chunk columns / 4) column groups, thread t owns group t % G and row slot t / G of
// R = 256 / G slots; it walks rows slot, slot + R, ... of the tile, CS_UNROLL rows at a time: the CS_UNROLL loads are
// issued before the first is consumed, the batch is reduced to (mean, M2) around its OWN mean and merged into the
// thread's running partial with the pairwise update (one fp64 division per batch and column instead of one per value).
// A group's four columns are 4g .. 4g+3, fetched as one 16-byte lane, when the span's base address, the row pitch and
// n_cols allow; else g, g + G, g + 2G, g + 3G, fetched as four 4-byte lanes — either way consecutive lanes read
// consecutive addresses of a row, and a column meets the same rows in the same order.  The R slot partials of a column
// are combined through LDS by a binary tree over the slot number.
//
// Workspace (fp64): level 0 | level 1 | ..., level l holding cnt_l partials of [m(C) | M2(C) | min(C) | max(C) | rho(C)];
// cnt_0 = tiles, cnt_{l+1} = ceil(cnt_l / CS_SWEEP), levels are kept while cnt_l > 1 (level 0 always).
//
// Affine pass.  out[i, c] = fl(fl(x - shift) / div) [then fl(. * mul)] on up to 8 column spans, one element per lane,
// each read and written once by the same lane (in place is safe); columns outside the spans are neither loaded nor
// stored.  A span moves as 16-byte lanes when its first column in both buffers, both pitches and its length allow.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace porl {

constexpr int CS_THREADS = 256;
constexpr int CS_TILE = 512;                       // rows per block
constexpr int CS_SWEEP = 64;                       // partials folded by one thread of the merge
constexpr int CS_UNROLL = 8;                       // rows in flight per thread
constexpr int CS_CHUNK = 4 * CS_THREADS;           // columns per block
constexpr int CS_STATS = 5;                        // doubles per column of a stored partial
constexpr int AF_MAX_SPANS = 8;
constexpr int AF_BLOCK_UNITS = 4096;               // lanes of work a block of the affine pass takes per step

// Workgroup barrier that retires LDS traffic only (qnet_fused.hpp): nothing below communicates through global memory
// between barriers, so outstanding global loads need not drain.
__device__ __forceinline__ void cs_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

struct CsAcc { double mean, m2, mn, mx, rho; };    // mean: the stored centre m; m2 about m; rho = sum (x - m)

__device__ __forceinline__ double cs_min(double a, double b) { return (b < a || b != b) ? b : a; }   // a NaN, once in, stays
__device__ __forceinline__ double cs_max(double a, double b) { return (b > a || b != b) ? b : a; }

// a (na values) <- a merged with b (nb values); either side may be empty
__device__ __forceinline__ void cs_merge(CsAcc& a, double na, const CsAcc& b, double nb) {
  if (nb == 0.0) return;
  if (na == 0.0) { a = b; return; }
  const double r = nb / (na + nb), d = b.mean - a.mean;
  const double c = a.mean + d * r, ea = a.mean - c, eb = b.mean - c;
  a.m2 = a.m2 + b.m2 + (na * ea * ea + nb * eb * eb) + 2.0 * (ea * a.rho + eb * b.rho);
  a.rho = (na * ea + nb * eb) + (a.rho + b.rho);
  a.mean = c;
  a.mn = cs_min(a.mn, b.mn);
  a.mx = cs_max(a.mx, b.mx);
}

// the statistics of x[0 .. m) (1 <= m <= CS_UNROLL) around their own mean, merged into a
__device__ __forceinline__ void cs_fold(CsAcc& a, double na, const float (&x)[CS_UNROLL], int m) {
  double sum = 0.0;
  CsAcc b;
  b.mn = b.mx = (double)x[0];
#pragma unroll
  for (int j = 0; j < CS_UNROLL; ++j)
    if (j < m) { const double v = (double)x[j]; sum += v; b.mn = cs_min(b.mn, v); b.mx = cs_max(b.mx, v); }
  b.mean = m == CS_UNROLL ? sum * (1.0 / CS_UNROLL) : sum / (double)m;      // a power of two: the product is the quotient
  b.rho = fma(-(double)m, b.mean, sum);            // exact: what the rounding of the quotient left over
  b.m2 = 0.0;
#pragma unroll
  for (int j = 0; j < CS_UNROLL; ++j)
    if (j < m) { const double e = (double)x[j] - b.mean; b.m2 += e * e; }
  cs_merge(a, na, b, (double)m);
}

// rows covered by partial i of a level whose partials span `span` rows each
__device__ __forceinline__ double cs_rows(long long i, long long span, long long n) {
  const long long lo = i * span, left = n - lo;
  return (double)(left < span ? left : span);
}

__device__ __forceinline__ void cs_put(double (&sh)[CS_STATS][CS_THREADS], int tid, const CsAcc& a) {
  sh[0][tid] = a.mean; sh[1][tid] = a.m2; sh[2][tid] = a.mn; sh[3][tid] = a.mx; sh[4][tid] = a.rho;
}

// base: column col0 of row 0.  VEC: 16-byte lanes (the host checked base, stride and n_cols).  Every load is bounded by
// n_rows and by the span; ws receives partial blockIdx.x of level 0.
template <bool VEC>
__global__ __launch_bounds__(CS_THREADS) void cs_tile_kernel(const float* __restrict__ base, long long stride, long long n_rows,
                                                             int n_cols, double* __restrict__ ws) {
  __shared__ double sh[4][CS_STATS][CS_THREADS];   // [column of the group][statistic][thread]
  __shared__ double shn[CS_THREADS];
  const int tid = threadIdx.x;
  const int chunk0 = blockIdx.y * CS_CHUNK;
  const int cc = n_cols - chunk0 < CS_CHUNK ? n_cols - chunk0 : CS_CHUNK;   // columns of this chunk
  const int G = (cc + 3) >> 2, R = CS_THREADS / G;
  const int g = tid % G, s = tid / G;
  const long long tile0 = (long long)blockIdx.x * CS_TILE;
  const int rows = n_rows - tile0 < CS_TILE ? (int)(n_rows - tile0) : CS_TILE;
  int col[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) col[k] = VEC ? 4 * g + k : g + k * G;
  CsAcc acc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { acc[k].mean = 0.0; acc[k].m2 = 0.0; acc[k].mn = 0.0; acc[k].mx = 0.0; acc[k].rho = 0.0; }
  double na = 0.0;
  if (s < R) {
    const float* __restrict__ p0 = base + tile0 * stride + chunk0;
    for (int r0 = s; r0 < rows; r0 += R * CS_UNROLL) {
      float x[4][CS_UNROLL];
#pragma unroll
      for (int j = 0; j < CS_UNROLL; ++j) {        // all loads first
        const int r = r0 + j * R;
        const bool in = r < rows;
        const float* __restrict__ p = p0 + (long long)(in ? r : r0) * stride;
        if (VEC) {
          const float4 v = in ? *reinterpret_cast<const float4*>(p + col[0]) : make_float4(0.f, 0.f, 0.f, 0.f);
          x[0][j] = v.x; x[1][j] = v.y; x[2][j] = v.z; x[3][j] = v.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) x[k][j] = in && col[k] < cc ? p[col[k]] : 0.f;
        }
      }
      const int left = (rows - r0 + R - 1) / R;
      const int m = left < CS_UNROLL ? left : CS_UNROLL;
#pragma unroll
      for (int k = 0; k < 4; ++k) cs_fold(acc[k], na, x[k], m);
      na += (double)m;
    }
  }
  // the R slot partials of every column, combined by a binary tree over the slot number
#pragma unroll
  for (int k = 0; k < 4; ++k) cs_put(sh[k], tid, acc[k]);
  shn[tid] = na;
  int h = 1;
  while (h < R) h <<= 1;
  for (h >>= 1; h >= 1; h >>= 1) {
    cs_barrier();
    if (s < h && s + h < R) {                      // reads slots [h, 2h), writes slots [0, h)
      const int o = tid + h * G;
      const double nb = shn[o];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        CsAcc b;
        b.mean = sh[k][0][o]; b.m2 = sh[k][1][o]; b.mn = sh[k][2][o]; b.mx = sh[k][3][o]; b.rho = sh[k][4][o];
        cs_merge(acc[k], na, b, nb);
        cs_put(sh[k], tid, acc[k]);
      }
      na += nb;
      shn[tid] = na;
    }
  }
  if (s == 0) {
    double* __restrict__ o = ws + (long long)blockIdx.x * CS_STATS * n_cols + chunk0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (col[k] < cc) {
        o[col[k]] = acc[k].mean; o[n_cols + col[k]] = acc[k].m2; o[2 * n_cols + col[k]] = acc[k].mn; o[3 * n_cols + col[k]] = acc[k].mx;
        o[4 * n_cols + col[k]] = acc[k].rho;
      }
  }
}

// out partial q = in partials [q * CS_SWEEP, ...) cut at cnt_in, folded in index order; `span` = rows per input partial.
// FINAL (cnt_out == 1, out = the caller's): [mean | M2 | min | max] with the residual folded in.
template <bool FINAL>
__global__ __launch_bounds__(CS_THREADS) void cs_merge_kernel(const double* __restrict__ in, double* __restrict__ out, long long cnt_in,
                                                              long long cnt_out, long long n_rows, long long span, int n_cols) {
  const long long idx = (long long)blockIdx.x * CS_THREADS + threadIdx.x;
  const long long q = idx / n_cols;
  const int c = (int)(idx - q * n_cols);
  if (q >= cnt_out) return;
  const long long first = q * CS_SWEEP;
  const long long last = first + CS_SWEEP < cnt_in ? first + CS_SWEEP : cnt_in;
  const long long C = n_cols;
  const double* __restrict__ p = in + first * CS_STATS * C + c;
  CsAcc a;
  a.mean = p[0]; a.m2 = p[C]; a.mn = p[2 * C]; a.mx = p[3 * C]; a.rho = p[4 * C];
  double na = cs_rows(first, span, n_rows);
#pragma unroll 4
  for (long long i = first + 1; i < last; ++i) {
    p += CS_STATS * C;
    CsAcc b;
    b.mean = p[0]; b.m2 = p[C]; b.mn = p[2 * C]; b.mx = p[3 * C]; b.rho = p[4 * C];
    const double nb = cs_rows(i, span, n_rows);
    cs_merge(a, na, b, nb);
    na += nb;
  }
  if (FINAL) {                                     // na = n_rows here
    const double m2 = a.m2 - a.rho * a.rho / na;
    out[c] = a.mean + a.rho / na; out[C + c] = m2 < 0.0 ? 0.0 : m2; out[2 * C + c] = a.mn; out[3 * C + c] = a.mx;
  } else {
    double* __restrict__ o = out + q * CS_STATS * C + c;
    o[0] = a.mean; o[C] = a.m2; o[2 * C] = a.mn; o[3 * C] = a.mx; o[4 * C] = a.rho;
  }
}

// ---- the affine pass ----------------------------------------------------------------------------------------------------
struct AfSpan { int col0, units, param0, flags, unit0; };       // flags bit 0: multiply, bit 1: 16-byte lanes

struct AfArgs {
  const float* rows; long long stride;
  float* out; long long out_stride;
  long long n_rows, n_blocks;
  const float *shift, *div, *mul;
  int n_spans, units_per_row, rows_per_block;
  AfSpan sp[AF_MAX_SPANS];
};

// fl(fl(x - s) / d), then fl(. * m).  __fdiv_rn is the IEEE round-to-nearest quotient: the build is plain -O3 without
// fast-math, so nothing may turn it into a multiplication by a reciprocal; contraction is off so that no two of the
// three operations can be fused into one rounding.
__device__ __forceinline__ float af_one(float x, float s, float d, float m, bool mul) {
#pragma clang fp contract(off)
  const float y = __fdiv_rn(__fsub_rn(x, s), d);
  return mul ? __fmul_rn(y, m) : y;
}

__global__ __launch_bounds__(CS_THREADS) void af_cols_kernel(const AfArgs a) {
  const int upr = a.units_per_row;
  for (long long rb = blockIdx.x; rb < a.n_blocks; rb += gridDim.x) {
    const long long row0 = rb * a.rows_per_block;
    const int nr = a.n_rows - row0 < a.rows_per_block ? (int)(a.n_rows - row0) : a.rows_per_block;
    const int total = nr * upr;
    for (int idx = threadIdx.x; idx < total; idx += CS_THREADS) {
      const int r = idx / upr, u = idx - r * upr;
      int col0 = a.sp[0].col0, param0 = a.sp[0].param0, flags = a.sp[0].flags, unit0 = 0;
#pragma unroll
      for (int k = 1; k < AF_MAX_SPANS; ++k)
        if (k < a.n_spans && u >= a.sp[k].unit0) { col0 = a.sp[k].col0; param0 = a.sp[k].param0; flags = a.sp[k].flags; unit0 = a.sp[k].unit0; }
      const bool mul = flags & 1;
      const long long row = row0 + r;
      if (flags & 2) {
        const int j = 4 * (u - unit0);
        const float4 x = *reinterpret_cast<const float4*>(a.rows + row * a.stride + col0 + j);
        const float* __restrict__ s = a.shift + param0 + j;
        const float* __restrict__ d = a.div + param0 + j;
        float m[4] = {1.f, 1.f, 1.f, 1.f};
        if (mul) { m[0] = a.mul[param0 + j]; m[1] = a.mul[param0 + j + 1]; m[2] = a.mul[param0 + j + 2]; m[3] = a.mul[param0 + j + 3]; }
        float4 y;
        y.x = af_one(x.x, s[0], d[0], m[0], mul); y.y = af_one(x.y, s[1], d[1], m[1], mul);
        y.z = af_one(x.z, s[2], d[2], m[2], mul); y.w = af_one(x.w, s[3], d[3], m[3], mul);
        *reinterpret_cast<float4*>(a.out + row * a.out_stride + col0 + j) = y;
      } else {
        const int j = u - unit0;
        const float x = a.rows[row * a.stride + col0 + j];
        const float m = mul ? a.mul[param0 + j] : 1.f;
        a.out[row * a.out_stride + col0 + j] = af_one(x, a.shift[param0 + j], a.div[param0 + j], m, mul);
      }
    }
  }
}

}  // namespace porl
