// Trajectory-level dataset passes of the reference (util/util.py:67-138) on a resident row store:
//
//   extract_done_makers (:83-87) / the episode walk of return_range (:67-80)  -> episode table (starts, ends)
//   return_range's per-episode sums and min / max                            -> ep_returns_kernel, ep_range_kernel
//   _sample_indces (:90-116)                                                 -> ep_pairs_kernel
//   rvs_sample_batch (:129-138)                                              -> ep_gather_pairs_kernel
//
// The table is a stream compaction of the rows that CLOSE an episode.  Row i closes one iff its done flag is set
// (d != 0.0f: NaN set, -0.0 clear) or, with a cap, iff it is the cap-th, 2*cap-th, ... row of its done-delimited run:
//     run_start(i) = 1 + max{ j < i : d[j] set }   (0 when there is none)        -- an exclusive MAX-scan of positions
//     closes(i)    = set(i) || (i - run_start(i) + 1) % cap == 0
//     rank(i)      = #{ j < i : closes(j) }                                       -- an exclusive SUM-scan
//     ends[rank(i)] = i,  starts[rank(i) + 1] = i + 1,  starts[0] = 0
//
// Launch structure.  No block ever waits for another block: every scan is block partials -> one block over the partials
// -> a second pass over the rows, as separate launches, and every loop's trip count follows from the arguments.
//   count:  ep_lastdone_kernel (cap only)  -> ep_scan_partials_kernel<MAX> (cap only, 1 wave)
//           -> ep_close_kernel<false>      -> ep_scan_partials_kernel<SUM> (1 wave; writes K and the trailing length)
//   fill:   ep_close_kernel<true>          (reads the carries and offsets the count left in the workspace)
// A block owns EP_TILE = EP_SUB x 256 consecutive rows and walks them as EP_SUB sub-tiles of one row per thread; the
// partial scan takes EP_SWEEP partials per sweep of its one wave.
//
// Workspace (int64): [0] K | [1] trailing rows | lastdone[nb] | carry[nb] | cnt[nb] | off[nb] | lastclose[nb], nb tiles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace porl {

constexpr int EP_THREADS = 256;
constexpr int EP_SUB = 4;
constexpr int EP_TILE = EP_THREADS * EP_SUB;       // rows per block
constexpr int EP_SWEEP = 64;                       // partials per sweep of the one-wave partial scan
constexpr int EP_RANGE_BLOCKS = 256;               // partials of the min / max reduction; its scratch is 4 int64 words each

struct EpFlags {
  const float* base; long long stride; long long n;
  __device__ __forceinline__ bool set(long long i) const { return i < n && base[i * stride] != 0.0f; }
};

template <bool MAX>
__device__ __forceinline__ long long ep_op(long long a, long long b) { return MAX ? (a > b ? a : b) : a + b; }

// Exclusive scan of one value per thread over a block of NW waves (identity `id`); `total` is the block's reduction.
// Every thread of the block must call it.  `sh` holds NW words and is free again on return.
template <bool MAX, int NW>
__device__ __forceinline__ long long ep_block_scan(long long v, long long id, long long* sh, long long& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long t = __shfl_up(inc, d);
    if (lane >= d) inc = ep_op<MAX>(inc, t);
  }
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  long long ex = __shfl_up(inc, 1);
  if (lane == 0) ex = id;
  long long pre = id;
  total = id;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const long long s = sh[w];
    if (w < wave) pre = ep_op<MAX>(pre, s);
    total = ep_op<MAX>(total, s);
  }
  __syncthreads();
  return ep_op<MAX>(pre, ex);
}

// lastdone[b] = the last set flag of tile b, or -1
__global__ __launch_bounds__(EP_THREADS) void ep_lastdone_kernel(const EpFlags f, long long* __restrict__ lastdone) {
  __shared__ long long sh[EP_THREADS / 64];
  const long long tile0 = (long long)blockIdx.x * EP_TILE;
  long long last = -1;
#pragma unroll
  for (int j = 0; j < EP_SUB; ++j) {
    const long long i = tile0 + j * EP_THREADS + threadIdx.x;
    if (f.set(i)) last = i;
  }
  long long total;
  (void)ep_block_scan<true, EP_THREADS / 64>(last, -1, sh, total);
  if (threadIdx.x == 0) lastdone[blockIdx.x] = total;
}

// out[b] = op over in[0 .. b) (exclusive), one wave walking all nb partials EP_SWEEP at a time.  The SUM instance is the
// last launch of the count: it also writes info[0] = K and info[1] = n - 1 - (last closing row), the trailing length.
template <bool MAX>
__global__ __launch_bounds__(EP_SWEEP) void ep_scan_partials_kernel(const long long* __restrict__ in, long long* __restrict__ out,
                                                                    long long nb, const long long* __restrict__ lastclose,
                                                                    long long* __restrict__ info, long long n) {
  __shared__ long long sh[1];
  const long long id = MAX ? -1 : 0;
  long long run = id, lc = -1;
  for (long long base = 0; base < nb; base += EP_SWEEP) {
    const long long idx = base + threadIdx.x;
    long long total;
    const long long ex = ep_block_scan<MAX, 1>(idx < nb ? in[idx] : id, id, sh, total);
    if (idx < nb) {
      out[idx] = ep_op<MAX>(run, ex);
      if (!MAX) { const long long c = lastclose[idx]; lc = c > lc ? c : lc; }
    }
    run = ep_op<MAX>(run, total);
  }
  if (!MAX) {
    long long total;
    (void)ep_block_scan<true, 1>(lc, -1, sh, total);
    if (threadIdx.x == 0) { info[0] = run; info[1] = n - 1 - total; }
  }
}

// The pass over the rows.  FILL = false: cnt[b] = closing rows of tile b, lastclose[b] = the last of them or -1.
// FILL = true: scatter them at off[b] + their rank inside the tile; K bounds every store.
template <bool FILL>
__global__ __launch_bounds__(EP_THREADS) void ep_close_kernel(const EpFlags f, long long cap, const long long* __restrict__ carry,
                                                              const long long* __restrict__ off, long long* __restrict__ cnt,
                                                              long long* __restrict__ lastclose, long long K,
                                                              long long* __restrict__ starts, long long* __restrict__ ends) {
  __shared__ long long sh[EP_THREADS / 64];
  const long long tile0 = (long long)blockIdx.x * EP_TILE;
  long long run_last = cap > 0 ? carry[blockIdx.x] : -1;       // the last set flag before this sub-tile
  long long run_cnt = FILL ? off[blockIdx.x] : 0;              // closing rows before this sub-tile
  long long last = -1;
  for (int j = 0; j < EP_SUB; ++j) {
    const long long i = tile0 + j * EP_THREADS + threadIdx.x;
    const bool set = f.set(i);
    bool closes = set;
    if (cap > 0) {                                             // block-uniform
      long long total;
      const long long ex = ep_block_scan<true, EP_THREADS / 64>(set ? i : -1, -1, sh, total);
      const long long len = i - (run_last > ex ? run_last : ex);          // rows of the run up to and including i
      closes = set || (i < f.n && len >= cap && len % cap == 0);
      run_last = run_last > total ? run_last : total;
    }
    long long total;
    const long long ex = ep_block_scan<false, EP_THREADS / 64>(closes ? 1 : 0, 0, sh, total);
    if (FILL) {
      const long long k = run_cnt + ex;
      if (closes && k < K) {
        ends[k] = i;
        if (k + 1 < K) starts[k + 1] = i + 1;
      }
    } else if (closes) {
      last = i;
    }
    run_cnt += total;
  }
  if (FILL) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && K > 0) starts[0] = 0;
  } else {
    long long total;
    (void)ep_block_scan<true, EP_THREADS / 64>(last, -1, sh, total);
    if (threadIdx.x == 0) { cnt[blockIdx.x] = run_cnt; lastclose[blockIdx.x] = total; }
  }
}

// returns[k] = 0.0 + r[starts[k]] + ... + r[ends[k]] in fp64, added IN ROW ORDER (the reference's `ep_ret += float(r)`
// on a Python float; any other association rounds differently).  One episode per wave: the wave fetches 64 rewards in
// parallel and adds them one after another through lane reads, so a long episode pays one memory latency per 64 rows.
__global__ __launch_bounds__(256) void ep_returns_kernel(const float* __restrict__ rew, long long stride, long long n,
                                                         const long long* __restrict__ starts, const long long* __restrict__ ends,
                                                         long long K, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
  for (long long k = wave; k < K; k += nwaves) {
    long long a = starts[k], b = ends[k];
    if (a < 0) a = 0;
    if (b >= n) b = n - 1;
    double acc = 0.0;
    for (long long c = a; c <= b; c += 64) {
      const long long i = c + lane;
      const float r = i <= b ? rew[i * stride] : 0.f;
      const int m = b - c + 1 < 64 ? (int)(b - c + 1) : 64;
      for (int j = 0; j < m; ++j) acc += (double)__shfl(r, j);
    }
    if (lane == 0) out[k] = acc;
  }
}

// Exact min / max over K doubles, NaNs set aside and reported.  Equal returns are equal bit for bit (a sum that starts
// from +0.0 is never -0.0), so which of them min() / max() keeps does not show.
struct EpRange { double mn, mx; int has, nan; };

__device__ __forceinline__ void ep_range_merge(EpRange& a, const EpRange& b) {
  if (b.has) {
    if (!a.has || b.mn < a.mn) a.mn = b.mn;
    if (!a.has || b.mx > a.mx) a.mx = b.mx;
    a.has = 1;
  }
  a.nan |= b.nan;
}

// FINAL = false: grid of <= EP_RANGE_BLOCKS blocks over vals[0 .. count) -> one partial per block in ws.
// FINAL = true:  one block over `count` partials in ws -> out[0] = min, out[1] = max, out[2] = 1.0 if a NaN was seen.
template <bool FINAL>
__global__ __launch_bounds__(256) void ep_range_kernel(const double* __restrict__ vals, long long count, long long* __restrict__ ws,
                                                       double* __restrict__ out) {
  __shared__ EpRange sh[256];
  EpRange r{0.0, 0.0, 0, 0};
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < count; k += (long long)gridDim.x * 256) {
    EpRange c;
    if (FINAL) {
      c.mn = __longlong_as_double(ws[k]); c.mx = __longlong_as_double(ws[EP_RANGE_BLOCKS + k]);
      c.has = (int)ws[2 * EP_RANGE_BLOCKS + k]; c.nan = (int)ws[3 * EP_RANGE_BLOCKS + k];
    } else {
      const double v = vals[k];
      c.mn = c.mx = v; c.nan = v != v; c.has = !c.nan;
    }
    ep_range_merge(r, c);
  }
  sh[threadIdx.x] = r;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { EpRange a = sh[threadIdx.x]; ep_range_merge(a, sh[threadIdx.x + s]); sh[threadIdx.x] = a; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const EpRange t = sh[0];
    if (FINAL) {
      const double qnan = __longlong_as_double(0x7FF8000000000000ll);
      out[0] = t.has ? t.mn : qnan;
      out[1] = t.has ? t.mx : qnan;
      out[2] = t.nan ? 1.0 : 0.0;
    } else {
      const int b = blockIdx.x;
      ws[b] = __double_as_longlong(t.mn); ws[EP_RANGE_BLOCKS + b] = __double_as_longlong(t.mx);
      ws[2 * EP_RANGE_BLOCKS + b] = t.has; ws[3 * EP_RANGE_BLOCKS + b] = t.nan;
    }
  }
}

// The draw of _sample_indces as a counter-based generator: splitmix64's output function on a key and a counter.
//   sm64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
//   key = sm64(seed ^ sm64(step)),  x_s(i) = sm64(key ^ sm64(3 i + s)) for stream s = 0 (traj), 1 (u1), 2 (u2)
//   traj = mulhi64(x_0, E),  u = (x >> 11) * 2^-53
__host__ __device__ __forceinline__ uint64_t ep_sm64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// t = floor(u * span) kept inside [0, hi]: with u on the 2^-53 grid in [0, 1) the clamp never acts (u * span < span, and a
// product that rounds up lands on the predecessor's integer part); it only keeps a caller's bad u inside the episode.
__device__ __forceinline__ long long ep_time_index(double u, long long span, long long hi) {
  const double f = floor(u * (double)span);
  if (!(f > 0.0)) return 0;
  return f >= (double)hi ? hi : (long long)f;
}

struct EpPairArgs {
  const long long* starts; const long long* lengths; long long E; int batch; uint64_t key;
  const long long* traj_in; const double* u1_in; const double* u2_in;
  long long* start; long long* goal; long long* traj_out; double* u1_out; double* u2_out;
};

// One thread per sample.  A given trajectory outside [0, E) yields start = goal = -1 (which the gather turns into a NaN
// row) instead of a read outside the table.
__global__ __launch_bounds__(256) void ep_pairs_kernel(const EpPairArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.batch) return;
  long long tr;
  double u1, u2;
  if (a.traj_in) {
    tr = a.traj_in[i]; u1 = a.u1_in[i]; u2 = a.u2_in[i];
  } else {
    const uint64_t c = 3ull * (uint64_t)i;
    tr = (long long)__umul64hi(ep_sm64(a.key ^ ep_sm64(c)), (uint64_t)a.E);
    u1 = (double)(ep_sm64(a.key ^ ep_sm64(c + 1)) >> 11) * 0x1.0p-53;
    u2 = (double)(ep_sm64(a.key ^ ep_sm64(c + 2)) >> 11) * 0x1.0p-53;
  }
  long long s = -1, g = -1;
  if (tr >= 0 && tr < a.E) {
    const long long len = a.lengths[tr], st = a.starts[tr];
    const long long hi = len > 0 ? len - 1 : 0;
    const long long t1 = ep_time_index(u1, hi, hi), t2 = ep_time_index(u2, len, hi);
    s = st + (t1 < t2 ? t1 : t2);
    g = st + (t1 < t2 ? t2 : t1);
  }
  a.start[i] = s;
  a.goal[i] = g;
  if (a.traj_out) a.traj_out[i] = tr;
  if (a.u1_out) a.u1_out[i] = u1;
  if (a.u2_out) a.u2_out[i] = u2;
}

// rvs_sample_batch in the wire format: out[i] = [ rows[start[i]][:S] | 0 | rows[goal[i]][:S] | 0 | rows[start[i]][2S+2:] ].
// One wave per batch row.  The first segment starts a row on both sides, so it moves as 16-byte lanes when the row
// pitches and bases allow; the others start at odd offsets (S + 1, 2S + 2 against 0 or S + 1) and move float by float.
// A start or goal outside [0, n_rows) makes the whole output row NaN.
__global__ __launch_bounds__(256) void ep_gather_pairs_kernel(const float* __restrict__ rows, long long row_stride, long long n_rows,
                                                              const long long* __restrict__ start, const long long* __restrict__ goal,
                                                              int batch, int S, int A, float* __restrict__ out, long long out_stride) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= batch) return;
  const long long si = start[i], gi = goal[i];
  float* dst = out + (long long)i * out_stride;
  const int W = 2 * S + 2 + A;
  if (si < 0 || si >= n_rows || gi < 0 || gi >= n_rows) {
    const float qnan = __int_as_float(0x7FC00000);
    for (int c = lane; c < W; c += 64) dst[c] = qnan;
    return;
  }
  const float* __restrict__ ss = rows + si * row_stride;
  const float* __restrict__ sg = rows + gi * row_stride;
  const bool vec = (row_stride & 3) == 0 && (out_stride & 3) == 0 &&
                   ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int S4 = vec ? S & ~3 : 0;
  for (int c = lane * 4; c < S4; c += 256) *reinterpret_cast<float4*>(dst + c) = *reinterpret_cast<const float4*>(ss + c);
  for (int c = S4 + lane; c < S; c += 64) dst[c] = ss[c];
  for (int c = lane; c < S; c += 64) dst[S + 1 + c] = sg[c];
  for (int c = lane; c < A; c += 64) dst[2 * S + 2 + c] = ss[2 * S + 2 + c];
  if (lane == 0) { dst[S] = 0.f; dst[2 * S + 1] = 0.f; }
}

}  // namespace porl
