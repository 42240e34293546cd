// Stable two-way partition of the rows of a resident store — the device side of generate_test_generlaization_data
// (util/util.py:219-238), which deletes every transition whose first two observation coordinates lie in a box.  Here
// nothing is deleted: the rows that are NOT held go to the front of one output buffer, the held rows behind them, both
// in input order, so the caller gets the training part and the held-out part from one copy of the store.
//
//     held(i)      = mask[i] != 0                                               form (a): a uint8 vector
//                  = x_lo <= r_i[cx] <= x_hi && y_lo <= r_i[cy] <= y_hi        form (b): fp32, inclusive, NaN -> not held
//     rank_kept(i) = #{ j < i : !held(j) }                                      -- an exclusive SUM-scan
//     dest(i)      = held(i) ? K + (i - rank_kept(i)) : rank_kept(i),   K = rank_kept(n)
//
// Launch structure (episodes.hpp): no block ever waits for another block, every loop's trip count follows from the
// arguments.
//   pt_count_kernel    cnt[b] = kept rows of tile b
//   pt_scan_kernel     (1 wave) off[b] = kept rows before tile b, info[0] = K, info[1] = n - K
//   pt_scatter_kernel  recomputes held(i) from the same inputs, ranks the tile, copies every row to dest(i)
// Form (b) stores no mask: the predicate costs two loads per row against a row copy of tens to hundreds of bytes, and a
// stored mask would be one more buffer to allocate, write and read back.
// A block owns PT_TILE = PT_SUB x 256 consecutive rows; the partial scan takes EP_SWEEP partials per sweep.
//
// Workspace (int64): [0] K | [1] n - K | cnt[nb] | off[nb], nb tiles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "episodes.hpp"

namespace porl {

constexpr int PT_THREADS = 256;
constexpr int PT_SUB = 2;
constexpr int PT_TILE = PT_THREADS * PT_SUB;       // rows per block

struct PtPred {
  const uint8_t* mask;                             // form (a), or null for form (b)
  const char* base; long long stride;              // the rows, stride in bytes
  int cx, cy; float x_lo, x_hi, y_lo, y_hi;
  long long n;
  __device__ __forceinline__ bool held(long long i) const {
    if (i >= n) return false;
    if (mask) return mask[i] != 0;
    const float* r = reinterpret_cast<const float*>(base + i * stride);
    const float x = r[cx], y = r[cy];
    return x >= x_lo && x <= x_hi && y >= y_lo && y <= y_hi;
  }
};

// Rows move as 16-byte lanes when both buffers, the input pitch and the row length allow, else as 32-bit words.
__host__ __device__ __forceinline__ bool pt_vec16(const void* base, long long stride, const void* out, long long row_bytes) {
  return ((reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(out) | (uintptr_t)stride | (uintptr_t)row_bytes) & 15) == 0;
}

// mask[i] = held(i) of form (b), for callers that compact several arrays by one predicate
__global__ __launch_bounds__(PT_THREADS) void pt_mask_kernel(const PtPred p, uint8_t* __restrict__ mask) {
  const long long i = (long long)blockIdx.x * PT_THREADS + threadIdx.x;
  if (i < p.n) mask[i] = p.held(i) ? 1 : 0;
}

__global__ __launch_bounds__(PT_THREADS) void pt_count_kernel(const PtPred p, long long* __restrict__ cnt) {
  __shared__ long long sh[PT_THREADS / 64];
  const long long tile0 = (long long)blockIdx.x * PT_TILE;
  long long kept = 0;
#pragma unroll
  for (int j = 0; j < PT_SUB; ++j) {
    const long long i = tile0 + j * PT_THREADS + threadIdx.x;
    if (i < p.n && !p.held(i)) ++kept;
  }
  long long total;
  (void)ep_block_scan<false, PT_THREADS / 64>(kept, 0, sh, total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// off[b] = cnt[0] + ... + cnt[b-1], one wave walking all nb partials EP_SWEEP at a time; info[0] = K, info[1] = n - K
__global__ __launch_bounds__(EP_SWEEP) void pt_scan_kernel(const long long* __restrict__ cnt, long long* __restrict__ off,
                                                           long long nb, long long* __restrict__ info, long long n) {
  __shared__ long long sh[1];
  long long run = 0;
  for (long long base = 0; base < nb; base += EP_SWEEP) {
    const long long idx = base + threadIdx.x;
    long long total;
    const long long ex = ep_block_scan<false, 1>(idx < nb ? cnt[idx] : 0, 0, sh, total);
    if (idx < nb) off[idx] = run + ex;
    run += total;
  }
  if (threadIdx.x == 0) { info[0] = run; info[1] = n - run; }
}

// `lpr` lanes copy one row (a power of two <= 64 chosen by the host from the row length), so a block moves
// PT_THREADS / lpr rows per pass and makes PT_TILE * lpr / PT_THREADS passes.  Every store is bounded by n.
__global__ __launch_bounds__(PT_THREADS) void pt_scatter_kernel(const PtPred p, const long long* __restrict__ off,
                                                                const long long* __restrict__ info, char* __restrict__ out,
                                                                long long* __restrict__ index, long long row_bytes, int lpr) {
  __shared__ long long sh[PT_THREADS / 64];
  __shared__ long long dest[PT_TILE];
  const long long tile0 = (long long)blockIdx.x * PT_TILE;
  const long long K = info[0];
  long long run = off[blockIdx.x];                 // kept rows before this sub-tile
#pragma unroll
  for (int j = 0; j < PT_SUB; ++j) {
    const long long i = tile0 + j * PT_THREADS + threadIdx.x;
    const bool in = i < p.n;
    const bool kept = in && !p.held(i);
    long long total;
    const long long rank = run + ep_block_scan<false, PT_THREADS / 64>(kept ? 1 : 0, 0, sh, total);
    dest[j * PT_THREADS + threadIdx.x] = !in ? -1 : kept ? rank : K + (i - rank);
    run += total;
  }
  __syncthreads();
  const bool vec = pt_vec16(p.base, p.stride, out, row_bytes);
  const int per_pass = PT_THREADS / lpr, sub = threadIdx.x / lpr, lane = threadIdx.x % lpr;
  for (int r = sub; r < PT_TILE; r += per_pass) {
    const long long d = dest[r];
    if (d < 0 || d >= p.n) continue;
    const char* __restrict__ src = p.base + (tile0 + r) * p.stride;
    char* __restrict__ dst = out + d * row_bytes;
    if (vec) {
      const int units = (int)(row_bytes >> 4);
      for (int c = lane; c < units; c += lpr) reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(src)[c];
    } else {
      const int units = (int)(row_bytes >> 2);
      for (int c = lane; c < units; c += lpr) reinterpret_cast<uint32_t*>(dst)[c] = reinterpret_cast<const uint32_t*>(src)[c];
    }
    if (index && lane == 0) index[d] = tile0 + r;
  }
}

}  // namespace porl
