// Prioritized replay inside the online loop (porl_per_record / porl_per_sample_slots / porl_per_update_f32,
// include/porl_hip.h; src/porl/train/dqn_per_trainer.py:127-175): the three launches of one PER environment step that
// is not the learn step itself.  The arithmetic is per_tree.hpp's, expression for expression, so every tree value,
// tree index and weight is bit-equal to what porl_per_update / porl_per_sample produce from the same inputs.
//
//   per_record_kernel        memory.add of ONE transition: the row travels in the kernel's arguments (like
//                            online_record_kernel) into slot `slot` of the five store arrays, the slot's leaf becomes
//                            (|td| + eps)^alpha and its ancestors are recomputed from their children, leaf to root, by
//                            one lane (a sequential chain of at most ceil(log2 capacity) + 1 fp64 additions).
//   per_sample_slots_kernel  per_sample_kernel without the priorities: tree indices, data slots (the rows the step
//                            kernel gathers itself), normalised weights and their mean as one fp32.  Its body is a
//                            device function of the uniform's source, which per_vector.hpp instantiates a second time.
//   per_update_f32_kernel    the priority write-back in one block: stamp -> last writer sets the leaf -> ancestors level
//                            by level, on the step kernel's fp32 |TD| widened to fp64.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "online.hpp"

namespace porl {

struct PerRecordArgs {
  float* states;
  float* next_states;
  int64_t* actions;
  float* rewards;
  float* dones;
  double* tree;
  int64_t capacity;
  int64_t slot;
  int64_t action;
  double td_error, eps, alpha;
  float reward, done;
  int S;
  float x[2 * ONL_MAX_RECORD_S];       // state | next_state
};

__global__ __launch_bounds__(256) void per_record_kernel(PerRecordArgs a) {
  const int64_t row = a.slot * a.S;
  for (int i = threadIdx.x; i < a.S; i += blockDim.x) {
    a.states[row + i] = a.x[i];
    a.next_states[row + i] = a.x[a.S + i];
  }
  if (threadIdx.x == 0) {
    a.actions[a.slot] = a.action;
    a.rewards[a.slot] = a.reward;
    a.dones[a.slot] = a.done;
    int64_t node = a.slot + a.capacity - 1;
    double v = pow(fabs(a.td_error) + a.eps, a.alpha);         // per_set_leaves_kernel's expression
    a.tree[node] = v;
    while (node != 0) {                                        // the sibling comes from memory, the path stays in v
      const int64_t parent = (node - 1) / 2;
      const int64_t sib = node == 2 * parent + 1 ? node + 1 : node - 1;
      const double s = a.tree[sib];
      v = node < sib ? v + s : s + v;                          // left + right, as per_propagate_kernel
      a.tree[parent] = v;
      node = parent;
    }
  }
}

struct PerSampleSlotsArgs {
  const double* tree; int64_t capacity;
  const double* u;             // (batch,) uniforms in [0, 1) from the host generator
  int batch; int64_t n_entries; double beta;
  int64_t* out_idx;            // tree indices
  int64_t* out_slots;          // data slots = tree index - (capacity - 1)
  float* out_w;                // importance weights, normalised by their maximum
  float* out_wmean;            // their mean: (sum_i raw_i) / max / batch, rounded once
  double* raw;                 // (batch,) scratch: the raw weights
};

// The body of per_sample_slots_kernel with the uniform of sample i as u_of(i): the one copy of the arithmetic, shared with
// per_sample_keyed_kernel (per_vector.hpp), which draws u_i itself.  One block of 256 lanes.
template <class UOf>
__device__ __forceinline__ void per_sample_slots_body(const PerSampleSlotsArgs& a, UOf u_of) {
  __shared__ double red[256];
  const int64_t size = 2 * a.capacity - 1;
  const double total = a.tree[0];
  const double segment = total / (double)a.batch;
  double wmax = 0.0;
  for (int i = threadIdx.x; i < a.batch; i += 256) {
    const double lo = segment * (double)i, hi = segment * (double)(i + 1);
    double s = lo + (hi - lo) * u_of(i);                      // random.uniform(a, b) = a + (b - a) * random()
    int64_t idx = 0;
    for (;;) {
      const int64_t left = 2 * idx + 1;
      if (left >= size) break;
      const double lv = a.tree[left];
      if (s <= lv) idx = left;
      else { s -= lv; idx = left + 1; }
    }
    const double p = a.tree[idx];
    a.out_idx[i] = idx;
    a.out_slots[i] = idx - (a.capacity - 1);
    const double w = pow((double)a.n_entries * (p / total), -a.beta);
    a.raw[i] = w;
    wmax = fmax(wmax, w);
  }
  red[threadIdx.x] = wmax;
  __syncthreads();                                            // also orders raw[] for the lanes below
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  wmax = red[0];
  for (int i = threadIdx.x; i < a.batch; i += 256) a.out_w[i] = (float)(a.raw[i] / wmax);
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int i = 0; i < a.batch; ++i) sum += a.raw[i];        // one fixed order
    *a.out_wmean = (float)(sum / wmax / (double)a.batch);
  }
}

__global__ __launch_bounds__(256) void per_sample_slots_kernel(const PerSampleSlotsArgs a) {
  per_sample_slots_body(a, [&a](int i) { return a.u[i]; });
}

// One block.  A tree index outside the leaves is skipped (nothing is read or written through it).
__global__ __launch_bounds__(1024) void per_update_f32_kernel(double* __restrict__ tree, const int64_t* __restrict__ tree_idx,
                                                              const float* __restrict__ td_abs, int n, int64_t capacity,
                                                              double eps, double alpha, int* __restrict__ stamp, int levels) {
  const int64_t first = capacity - 1, size = 2 * capacity - 1;
  const int nt = blockDim.x;
  for (int i = threadIdx.x; i < n; i += nt) {
    const int64_t t = tree_idx[i];
    if (t >= first && t < size) atomicMax(&stamp[t - first], i + 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += nt) {
    const int64_t t = tree_idx[i];
    if (t < first || t >= size) continue;
    if (__hip_atomic_load(&stamp[t - first], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i + 1) {
      tree[t] = pow(fabs((double)td_abs[i]) + eps, alpha);
      stamp[t - first] = 0;
    }
  }
  __syncthreads();
  // Leaves sit at two depths when capacity is not a power of two, so within one iteration a lane on a shallower path
  // can read a child that a lane on a deeper path is writing (a stale sum, never a torn one).  It cannot survive: the
  // deeper lane reaches that same parent one iteration later, after the barrier, with both children settled, and
  // writes it last.  Every ancestor therefore ends as the exact sum of its final children (per_propagate_kernel alike).
  for (int base = 0; base < n; base += nt) {
    const int i = base + threadIdx.x;
    int64_t node = i < n ? tree_idx[i] : 0;
    if (node < first || node >= size) node = 0;
    for (int l = 0; l < levels; ++l) {
      if (node != 0) {
        node = (node - 1) / 2;
        tree[node] = tree[2 * node + 1] + tree[2 * node + 2];
      }
      __syncthreads();
    }
  }
}

}  // namespace porl
