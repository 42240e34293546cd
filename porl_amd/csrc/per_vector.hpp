// Prioritized replay for a loop that writes N rows per launch and never returns to the host (porl_per_fill_range /
// porl_per_sample_keyed, include/porl_hip.h; train/vector_per.py).  Both kernels are pinned bit for bit to kernels already in
// the tree: the fill to per_set_leaves_kernel + per_propagate_kernel (per_tree.hpp), the sampler to per_sample_slots_kernel
// (per_online.hpp), whose body it calls.
//
//   per_fill_range_kernel    memory.add(td_error, ...) for the n data slots (first_slot + i) % capacity: each leaf becomes
//                            (|td| + eps)^alpha, every ancestor of one of them is recomputed as left + right.  The leaves are
//                            one contiguous run of tree indices (two when the ring wraps), and the parents of a contiguous run
//                            [a, b] are the contiguous run [(a-1)/2, (b-1)/2]: the kernel walks RUNS toward the root, about
//                            2n + 4*levels node writes, where n leaf-to-root paths cost n*levels.
//   per_sample_keyed_kernel  per_sample_slots_kernel with u_i drawn in the kernel from the counter stream (seed, draw, i).
//
// Order of the passes.  When capacity is not a power of two the leaves sit at two depths, D - 1 (tree indices below 2^D - 1)
// and D, so a run of leaves can cross from the tail of level D - 1 to the head of level D.  The host therefore cuts every
// run at 2^D - 1: each piece lies inside ONE level, and so does each of its parent runs.  The kernel then goes level by level
// from the deepest: in pass d it writes the nodes of depth d that are parents of a piece at depth d + 1, and a barrier ends
// the pass.  A node of depth d is thus written only after every node of depth d + 1 is final (the leaves of depth D - 1 are
// final before the first pass), so each ancestor is the exact fp64 sum of its final children the one time it is written per
// piece.  Two pieces can name the same parent (the two halves of a cut run meet at one node, a wrapped ring's two runs
// share the path near the root): both lanes read the same final children and store the same bits.
//
// One block.  Nothing here waits on another block, so nothing can hang; a block of 1024 lanes writes the 2n nodes of
// n = 65536 in 128 strided passes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "episodes.hpp"     // ep_sm64
#include "per_online.hpp"   // per_sample_slots_body

namespace porl {

constexpr int PER_FILL_MAX_RUNS = 4;                 // two runs (a wrapped ring), each cut once at the level boundary

struct PerFillArgs {
  double* tree;
  int64_t capacity, first_slot, n;
  double td_error, eps, alpha;
  int n_runs;                                        // pieces of leaves, each inside one level
  int top;                                           // depth of the deepest leaf
  int64_t lo[PER_FILL_MAX_RUNS], hi[PER_FILL_MAX_RUNS];   // tree indices, inclusive
  int depth[PER_FILL_MAX_RUNS];
};

// The pieces of the leaves of slots (first_slot + i) % capacity, i < n, cut at the ring's end and at the level boundary
// 2^top - 1.  Host code: no device call.  1 <= n <= capacity, 0 <= first_slot < capacity, top = depth of leaf 2*capacity - 2.
inline void per_fill_plan(PerFillArgs* a) {
  const int64_t first = a->capacity - 1, boundary = (int64_t(1) << a->top) - 1;
  a->n_runs = 0;
  auto add = [&](int64_t lo, int64_t hi) {           // a run of leaves -> at most two pieces
    if (lo < boundary) {
      a->lo[a->n_runs] = lo; a->hi[a->n_runs] = hi < boundary ? hi : boundary - 1; a->depth[a->n_runs++] = a->top - 1;
    }
    if (hi >= boundary) {
      a->lo[a->n_runs] = lo > boundary ? lo : boundary; a->hi[a->n_runs] = hi; a->depth[a->n_runs++] = a->top;
    }
  };
  const int64_t end = a->first_slot + a->n;          // one past the last slot, before wrapping
  if (end <= a->capacity) {
    add(first + a->first_slot, first + end - 1);
  } else {
    add(first + a->first_slot, first + a->capacity - 1);
    add(first, first + (end - a->capacity) - 1);
  }
}

__global__ __launch_bounds__(1024) void per_fill_range_kernel(const PerFillArgs a) {
  const int nt = blockDim.x;
  const int64_t first = a.capacity - 1;
  const double v = pow(fabs(a.td_error) + a.eps, a.alpha);    // per_set_leaves_kernel's expression
  for (int64_t i = threadIdx.x; i < a.n; i += nt) {
    int64_t slot = a.first_slot + i;
    if (slot >= a.capacity) slot -= a.capacity;
    a.tree[first + slot] = v;
  }
  __syncthreads();
  int64_t lo[PER_FILL_MAX_RUNS], hi[PER_FILL_MAX_RUNS];
  int depth[PER_FILL_MAX_RUNS];
#pragma unroll
  for (int r = 0; r < PER_FILL_MAX_RUNS; ++r) {
    lo[r] = a.lo[r]; hi[r] = a.hi[r]; depth[r] = r < a.n_runs ? a.depth[r] : -1;
  }
  for (int d = a.top - 1; d >= 0; --d) {                      // pass d writes nodes of depth d; uniform across the block
#pragma unroll
    for (int r = 0; r < PER_FILL_MAX_RUNS; ++r) {
      if (depth[r] != d + 1) continue;
      lo[r] = (lo[r] - 1) / 2; hi[r] = (hi[r] - 1) / 2; depth[r] = d;
      for (int64_t p = lo[r] + threadIdx.x; p <= hi[r]; p += nt)
        a.tree[p] = a.tree[2 * p + 1] + a.tree[2 * p + 2];    // left + right, as per_propagate_kernel
    }
    __syncthreads();
  }
}

// Stream tag of the keyed sampler: key = sm64(seed ^ PER_KEY_TAG).  PER_KEY_TAG = sm64(0x5045524B45594544), the ASCII bytes
// "PERKEYED".  The exploration draws of qnet_select_kernel and the reset draws of the simulator key their streams by
// sm64(seed ^ sm64(e)) with a robot index e <= 2^40 + 2^24; sm64 is a bijection and 0x5045524B45594544 is no such index, so
// no robot's key is this one under the same seed.  sample_indices builds 32-bit Feistel round keys from (seed, step) by
// another mixer and shares no value with this stream.
constexpr uint64_t PER_KEY_TAG = 0xF08CDF1E9B01AC12ull;
constexpr int64_t PER_KEYED_MAX_DRAW = (int64_t(1) << 32) - 1;  // draw rides in the high 32 bits of the counter, i in the low

__host__ __device__ __forceinline__ uint64_t per_keyed_key(uint64_t seed) { return ep_sm64(seed ^ PER_KEY_TAG); }

__device__ __forceinline__ double per_keyed_u(uint64_t key, uint64_t draw, int i) {
  return (double)(ep_sm64(key ^ ep_sm64((draw << 32) | (uint64_t)(uint32_t)i)) >> 11) * 0x1.0p-53;
}

__global__ __launch_bounds__(256) void per_sample_keyed_kernel(const PerSampleSlotsArgs a, uint64_t key, uint64_t draw) {
  per_sample_slots_body(a, [key, draw](int i) { return per_keyed_u(key, draw, i); });
}

}  // namespace porl
