// The labelling pass of the reference (preprocess.py:11-68 `preprocessing`, planner dataloader/a_star.py:8-221) as one
// workgroup per transition row, the whole problem in LDS:
//
//   scan (n_beams ranges) -> obstacle points -> occupancy BITMAP (points inflated by the robot radius) -> exact
//   8-connected shortest distance start -> goal -> path_len = nodes on a cheapest path -> value = table[path_len]
//
// Why no A*: the label depends only on len(rx).  A cheapest path costs a + b*sqrt(2) (a axis moves, b diagonal moves);
// sqrt(2) is irrational, so all cheapest paths share (a, b) and len = a + b + 1 does not depend on the planner's
// tie-breaking.  Distances are therefore kept as EXACT integer pairs, packed a << 16 | b in one uint32 per cell, and
// two pairs are compared through a + b*sqrt(2) evaluated afresh in fp64 from the integers — never an accumulated float.
// Distinct pairs with a + b < 65536 differ by |da^2 - 2 db^2| / |da + db*sqrt(2)| >= 1 / (65536 * 2.42) = 6e-6; the fp64
// evaluation (one conversion pair, one fma) is good to 1e-11, so the comparison is exact.
//
// Relaxation is pull-style and in place: every cell is written only by the thread that owns it, with the minimum over
// its 8 neighbours; blocked cells and the one-cell halo keep "unreached" for ever, so they never offer a candidate and
// no bounds or occupancy test is left in the sweep.  A thread may read a neighbour's value of this sweep or of the last:
// harmless — every value ever held is the (a, b) of a real path, values only decrease, and the only fixpoint is the
// true distance field.  Sweeps repeat until one changes nothing, or until the goal's pair is provably final (see the
// loop); the loop is bounded by the number of cells (a sweep that changes something settles at least one more cell),
// and a row that reaches the bound is reported NOT_CONVERGED.
//
// LDS (dynamic): dist[(W+2)*(H+2)] uint32 | occ[ceil((W+2)*(H+2)/32)] uint32 — 82 416 + 2 576 bytes at the reference's
// 200 x 100 grid, i.e. one workgroup per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace porl {

constexpr int AS_THREADS = 1024;
constexpr int AS_MAX_CELLS_PER_THREAD = 64;                  // the per-thread ownership mask is one uint64
constexpr int AS_MAX_PADDED_CELLS = AS_THREADS * AS_MAX_CELLS_PER_THREAD;
constexpr int AS_MAX_PAIR = 65534;                           // a + b of any path must stay below the "unreached" pair
constexpr int AS_MAX_LDS_BYTES = 160 * 1024 - 1024;          // beside ~64 bytes of static LDS
constexpr uint32_t AS_UNREACHED = 0xFFFFFFFFu;               // costs more than any pair a path can have

enum AstarStatus : int32_t {
  AS_LABELLED = 0, AS_TOO_CLOSE = 1, AS_GOAL_IS_START = 2, AS_GOAL_OFF_GRID = 3, AS_GOAL_BLOCKED = 4, AS_UNREACHABLE = 5,
  AS_NON_FINITE = 6, AS_NOT_CONVERGED = 7
};

// what the host derives from porl_astar_params (porl_api.hip: astar_plan)
struct AstarGrid {
  double res, rr, min_x, min_y, range_lo, range_hi;
  int32_t w, h, pw, pcells;            // grid, padded row pitch w + 2, padded cells (w + 2) * (h + 2)
  int32_t start_ix, start_iy;
  int32_t n_beams, pose_off, heading_off, goal_off;
  int32_t max_sweeps;
};

inline size_t astar_lds_bytes(int64_t pcells) { return (size_t)(pcells + (pcells + 31) / 32) * sizeof(uint32_t); }

__device__ __forceinline__ double as_cost(uint32_t v) {
  return fma((double)(v & 0xFFFFu), 1.4142135623730951, (double)(v >> 16));
}

// Blocks the cells whose centre lies within rr of the point (px, py).  Only the point's bounding box in cell indices is
// visited (one cell of slack each way for the rounding of the box itself); the in/out decision is the reference's:
// centre = index * resolution + min (a product, then a sum: no fused multiply-add), hypot(dx, dy) <= rr.
__device__ inline void as_mark_point(const AstarGrid& g, double px, double py, uint32_t* occ) {
#pragma clang fp contract(off)
  const double fx0 = floor((px - g.rr - g.min_x) / g.res) - 1.0, fx1 = ceil((px + g.rr - g.min_x) / g.res) + 1.0;
  const double fy0 = floor((py - g.rr - g.min_y) / g.res) - 1.0, fy1 = ceil((py + g.rr - g.min_y) / g.res) + 1.0;
  const int ix0 = (int)fmin(fmax(fx0, 0.0), (double)g.w), ix1 = (int)fmin(fmax(fx1, -1.0), (double)(g.w - 1));
  const int iy0 = (int)fmin(fmax(fy0, 0.0), (double)g.h), iy1 = (int)fmin(fmax(fy1, -1.0), (double)(g.h - 1));
  for (int ix = ix0; ix <= ix1; ++ix) {
    const double x = (double)ix * g.res + g.min_x;
    for (int iy = iy0; iy <= iy1; ++iy) {
      const double y = (double)iy * g.res + g.min_y;
      if (hypot(px - x, py - y) <= g.rr) {
        const int p = (iy + 1) * g.pw + ix + 1;                 // 0 <= p < pcells: ix, iy are clamped to the grid
        atomicOr(&occ[p >> 5], 1u << (p & 31));
      }
    }
  }
}

// Goal cell of the row: g = R(heading) (goal - pose), cell = rint((g - min) / resolution) — rint rounds half to even,
// as Python's round.  Returns the status that ends the row here, or AS_LABELLED with the cell in (ix, iy).
__device__ inline int as_goal_cell(const AstarGrid& g, const float* row, int* ix, int* iy) {
#pragma clang fp contract(off)
  const double hd = (double)row[g.heading_off];
  const double dx = (double)row[g.goal_off] - (double)row[g.pose_off];
  const double dy = (double)row[g.goal_off + 1] - (double)row[g.pose_off + 1];
  const double c = cos(hd), s = sin(hd);
  const double gx = c * dx + s * dy, gy = -s * dx + c * dy;
  const double fx = rint((gx - g.min_x) / g.res), fy = rint((gy - g.min_y) / g.res);
  if (!isfinite(fx) || !isfinite(fy)) return AS_NON_FINITE;
  if (fx == (double)g.start_ix && fy == (double)g.start_iy) return AS_GOAL_IS_START;
  if (fx < 0.0 || fx >= (double)g.w || fy < 0.0 || fy >= (double)g.h) return AS_GOAL_OFF_GRID;
  *ix = (int)fx;
  *iy = (int)fy;
  return AS_LABELLED;
}

__global__ __launch_bounds__(AS_THREADS) void astar_label_kernel(const float* __restrict__ rows, long row_stride,
                                                                 AstarGrid g, const double* __restrict__ beam_dirs,
                                                                 const float* __restrict__ value_table,
                                                                 float* __restrict__ value, int32_t* __restrict__ path_len,
                                                                 int32_t* __restrict__ status, int32_t* __restrict__ sweeps) {
  extern __shared__ uint32_t as_lds[];
  uint32_t* dist = as_lds;                  // [pcells], padded (iy + 1) * pw + ix + 1
  uint32_t* occ = as_lds + g.pcells;        // [ceil(pcells / 32)] bits, same index
  __shared__ int s_flag[3];                 // what a sweep found, rotating so that one barrier per sweep is enough
  __shared__ int s_nan, s_close, s_goal[3];

  const int tid = threadIdx.x;
  const long r = blockIdx.x;
  const float* row = rows + r * row_stride;
  const int occ_words = (g.pcells + 31) >> 5;

  if (tid == 0) { s_nan = 0; s_close = 0; s_flag[0] = s_flag[1] = s_flag[2] = 0; }
  for (int i = tid; i < occ_words; i += AS_THREADS) occ[i] = 0u;
  for (int i = tid; i < g.pcells; i += AS_THREADS) dist[i] = AS_UNREACHED;
  __syncthreads();

  // row filter — scan.min() < rr with numpy's min: one NaN beam makes the minimum NaN and the comparison false
  for (int i = tid; i < g.n_beams; i += AS_THREADS) {
    const double d = (double)row[i];
    if (d != d) s_nan = 1;
    else if (d < g.rr) s_close = 1;
  }
  if (tid == 0) {
    int ix = 0, iy = 0;
    s_goal[0] = as_goal_cell(g, row, &ix, &iy);
    s_goal[1] = ix;
    s_goal[2] = iy;
  }
  __syncthreads();
  int st = (s_close && !s_nan) ? (int)AS_TOO_CLOSE : s_goal[0];
  if (st != AS_LABELLED) {                                     // uniform over the workgroup
    if (tid == 0) { status[r] = st; path_len[r] = 0; value[r] = 0.0f; if (sweeps) sweeps[r] = 0; }
    return;
  }
  const int gidx = (s_goal[2] + 1) * g.pw + s_goal[1] + 1;
  const int sidx = (g.start_iy + 1) * g.pw + g.start_ix + 1;

  // occupancy: one kept beam per thread
  for (int i = tid; i < g.n_beams; i += AS_THREADS) {
    const double d = (double)row[i];
    if (d < g.range_hi && d > g.range_lo) as_mark_point(g, beam_dirs[2 * i] * d, beam_dirs[2 * i + 1] * d, occ);
  }
  __syncthreads();
  if ((occ[gidx >> 5] >> (gidx & 31)) & 1u) {                  // uniform
    if (tid == 0) { status[r] = AS_GOAL_BLOCKED; path_len[r] = 0; value[r] = 0.0f; if (sweeps) sweeps[r] = 0; }
    return;
  }

  // cells tid, tid + 1024, ... of the padded array are this thread's; bit k of `own`: cell k is interior, unblocked and
  // not the start (which holds (0, 0) for good, blocked or not: the reference never verifies the start node)
  uint64_t own = 0;
  for (int k = 0, idx = tid; idx < g.pcells; ++k, idx += AS_THREADS) {
    const int px = idx % g.pw, py = idx / g.pw;
    const bool interior = px >= 1 && px <= g.w && py >= 1 && py <= g.h;
    const bool blocked = (occ[idx >> 5] >> (idx & 31)) & 1u;
    if (interior && !blocked && idx != sidx) own |= uint64_t(1) << k;
  }
  if (tid == 0) dist[sidx] = 0u;
  __syncthreads();

  const int pw = g.pw;
  int sweep = 0;
  bool converged = false;
  while (sweep < g.max_sweeps) {
    bool changed = false;
    for (uint64_t m = own; m; m &= m - 1) {
      const int idx = tid + __builtin_ctzll(m) * AS_THREADS;    // interior: all 8 neighbours are inside the padded array
      const uint32_t cur = dist[idx];
      uint32_t va = dist[idx - 1], vd = dist[idx - pw - 1];
      double ca = as_cost(va), cd = as_cost(vd);
      uint32_t v;
      double c;
      v = dist[idx + 1];      c = as_cost(v); if (c < ca) { ca = c; va = v; }
      v = dist[idx - pw];     c = as_cost(v); if (c < ca) { ca = c; va = v; }
      v = dist[idx + pw];     c = as_cost(v); if (c < ca) { ca = c; va = v; }
      v = dist[idx - pw + 1]; c = as_cost(v); if (c < cd) { cd = c; vd = v; }
      v = dist[idx + pw - 1]; c = as_cost(v); if (c < cd) { cd = c; vd = v; }
      v = dist[idx + pw + 1]; c = as_cost(v); if (c < cd) { cd = c; vd = v; }
      uint32_t best = cur;
      double cb = as_cost(cur);
      if (va != AS_UNREACHED) { v = va + 0x10000u; c = as_cost(v); if (c < cb) { cb = c; best = v; } }   // one more axis move
      if (vd != AS_UNREACHED) { v = vd + 1u;       c = as_cost(v); if (c < cb) { cb = c; best = v; } }   // one more diagonal
      if (best != cur) { dist[idx] = best; changed = true; }
    }
    // flag[sweep % 3] collects this sweep (bit 0: a cell changed, bit 1: the goal is final); the slot after it is cleared
    // now — its last readers passed the previous barrier
    if (tid == 0) {
      s_flag[(sweep + 1) % 3] = 0;
      // After s sweeps every cell holds at most the cost of its cheapest path of <= s moves (Bellman-Ford; reading a
      // neighbour's newer value only helps).  A cheapest path to the goal has n* = a* + b* <= a* + b* sqrt(2) = c* moves,
      // and c* <= c', the cost of the pair the goal holds now (or held a sweep ago: larger still).  So once the sweeps
      // done reach c', the goal's pair is final and the rest of the field is of no interest.
      const uint32_t vg = dist[gidx];
      if (vg != AS_UNREACHED && (double)(sweep + 1) >= as_cost(vg)) atomicOr(&s_flag[sweep % 3], 2);
    }
    if (changed) atomicOr(&s_flag[sweep % 3], 1);
    __syncthreads();
    const int flag = s_flag[sweep % 3];
    ++sweep;
    if (flag != 1) { converged = true; break; }           // nothing changed, or the goal is final
  }

  if (tid == 0) {
    const uint32_t v = dist[gidx];
    int s = AS_LABELLED, n = 0;
    if (!converged) s = AS_NOT_CONVERGED;
    else if (v == AS_UNREACHED) s = AS_UNREACHABLE;
    else n = (int)(v >> 16) + (int)(v & 0xFFFFu) + 1;            // <= w * h: inside the value table
    status[r] = s;
    path_len[r] = n;
    value[r] = n ? value_table[n] : 0.0f;
    if (sweeps) sweeps[r] = sweep;
  }
}

}  // namespace porl
