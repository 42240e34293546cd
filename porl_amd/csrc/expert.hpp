// An A* expert for the lidar navigation task, planned on the device (porl_nav_rasterize / porl_nav_expert): the device form
// of the reference's dataloader/a_star.py `AStarPlanner.planning`, for N robots per call, with no read-back.
//
//   world (segments, circles) -> occupancy BITMAP of a w x h grid, once per world          nav_rasterize_kernel
//   goal of robot i -> exact 8-connected distance field from the goal cell, cached          nav_field_kernel
//   pose of robot i -> descent of its field -> waypoint (and path) -> command / scores      nav_steer_kernel
//
// Conventions (csrc/astar.hpp's, which are the reference's): the centre of cell (ix, iy) is ix * res + min_x, iy * res +
// min_y — a product, then a sum, no fused multiply-add (calc_grid_position); the cell of a position is rint((x - min_x) /
// res), half to even (calc_xy_index); padded index (iy + 1) * (w + 2) + ix + 1 with a one-cell halo; a distance is the
// exact pair a << 16 | b (a axis moves, b diagonal moves), compared through as_cost.  The field grows from the GOAL, so
// one field serves a robot for as long as its goal cell stays: tag[i] = iy * w + ix + 1 of the goal cell whose field row i
// of the cache holds, 0 for none, -1 when the sweep bound was reached.
//
// Descent: neighbours in the reference's motion order (1,0) (0,1) (-1,0) (0,-1) (-1,-1) (-1,1) (1,-1) (1,1); from a reached
// cell c that is not the goal the next cell is the first neighbour n with field[n] + move == field[c] as integers (move =
// 0x10000 for an axis step, 1 for a diagonal).  At the fixpoint such a neighbour exists.  Only integers are compared, so a
// host restatement walks the same cells.
//
// fp64 geometry with contraction off (NAV_EXACT); every loop bounded in the code; no global atomics, no communication
// between workgroups; every global write is a plain vector store.
#pragma once
#include "astar.hpp"
#include "navsim_discrete.hpp"   // NAV_EXACT, SELECT_MAX_ACTIONS

namespace porl {

constexpr int EX_RASTER_THREADS = 256;
constexpr int EX_STEER_THREADS = 256;

enum ExpertStatus : int32_t {
  EX_OK = 0, EX_NO_FIELD = 1, EX_GOAL_OFF_GRID = 2, EX_GOAL_BLOCKED = 3, EX_NON_FINITE = 4, EX_NOT_CONVERGED = 5
};

// what the host derives from porl_nav_grid (expert_api.inc: expert_plan)
struct ExpertGrid {
  double res, inflate, min_x, min_y;
  int32_t w, h, pw, pcells;            // grid, padded row pitch w + 2, padded cells (w + 2) * (h + 2)
  int32_t max_sweeps;
};

// Cell of a position: EX_OK with the cell in (ix, iy), EX_NON_FINITE, or EX_GOAL_OFF_GRID for "off the grid".
__device__ __forceinline__ int ex_cell(const ExpertGrid& g, double x, double y, int* ix, int* iy) {
  NAV_EXACT
  const double fx = rint((x - g.min_x) / g.res), fy = rint((y - g.min_y) / g.res);
  if (!isfinite(fx) || !isfinite(fy)) return EX_NON_FINITE;
  if (fx < 0.0 || fx >= (double)g.w || fy < 0.0 || fy >= (double)g.h) return EX_GOAL_OFF_GRID;
  *ix = (int)fx;
  *iy = (int)fy;
  return EX_OK;
}

__device__ __forceinline__ bool ex_bit(const uint32_t* occ, int p) { return (occ[p >> 5] >> (p & 31)) & 1u; }

// motion k of the reference's motion model: dx + 1, dy + 1 packed two bits each
__device__ __forceinline__ int ex_dx(int k) { return (int)((0xA046u >> (2 * k)) & 3u) - 1; }
__device__ __forceinline__ int ex_dy(int k) { return (int)((0x8819u >> (2 * k)) & 3u) - 1; }

// ---- porl_nav_rasterize -------------------------------------------------------------------------------------------------
// One thread per padded cell.  A cell is blocked iff its centre lies within `inflate` of a primitive; halo cells read 0.
// A wave's 64 decisions are one ballot; lanes 0 and 1 store its two words.  The last wave's ballot may straddle the end of
// the bitmap: lanes past pcells vote 0 and a word past n_words is not stored.
__global__ __launch_bounds__(EX_RASTER_THREADS) void nav_rasterize_kernel(const float* __restrict__ segments, int M,
                                                                          const float* __restrict__ circles, int C, ExpertGrid g,
                                                                          uint32_t* __restrict__ occ, int n_words) {
  NAV_EXACT
  const int p = blockIdx.x * EX_RASTER_THREADS + threadIdx.x;
  bool blocked = false;
  if (p < g.pcells) {
    const int px = p % g.pw, py = p / g.pw;
    if (px >= 1 && px <= g.w && py >= 1 && py <= g.h) {
      const double cx = (double)(px - 1) * g.res + g.min_x, cy = (double)(py - 1) * g.res + g.min_y;
      for (int k = 0; k < M && !blocked; ++k) {
        const double ax = (double)segments[4 * k], ay = (double)segments[4 * k + 1];
        const double ex = (double)segments[4 * k + 2] - ax, ey = (double)segments[4 * k + 3] - ay;
        const double ee = ex * ex + ey * ey;
        double qx = ax, qy = ay;                                  // e . e == 0: the segment is a point
        if (ee != 0.0) {
          double t = ((cx - ax) * ex + (cy - ay) * ey) / ee;
          t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
          qx = ax + t * ex;
          qy = ay + t * ey;
        }
        blocked = hypot(cx - qx, cy - qy) <= g.inflate;
      }
      for (int k = 0; k < C && !blocked; ++k) {
        const double d = hypot(cx - (double)circles[3 * k], cy - (double)circles[3 * k + 1]) - (double)circles[3 * k + 2];
        blocked = d <= g.inflate;
      }
    }
  }
  const unsigned long long votes = __ballot(blocked);
  const int lane = threadIdx.x & 63;
  const int word = ((p - lane) >> 5) + lane;                      // the wave's cells start at a multiple of 64
  if (lane < 2 && word < n_words) occ[word] = (uint32_t)(votes >> (32 * lane));
}

// One pull sweep over the cells bit k of `own` names (cell tid + k * AS_THREADS of the padded array, all interior, so all
// 8 neighbours are inside it): every such cell takes the cheapest of its own pair and its neighbours' pairs plus one
// move.  Returns whether a cell of this thread changed.  A second copy of the loop body of astar_label_kernel: sharing
// one function cost the labeller three scalar instructions per cell and about 1 % of its rate.
__device__ __forceinline__ bool ex_sweep(uint32_t* dist, uint64_t own, int tid, int pw) {
  bool changed = false;
  for (uint64_t m = own; m; m &= m - 1) {
    const int idx = tid + __builtin_ctzll(m) * AS_THREADS;
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
  return changed;
}

// ---- porl_nav_expert, first launch: the distance field of a robot whose goal cell changed ------------------------------------
// One workgroup per robot; dynamic LDS as astar_label_kernel's: dist[pcells] | occ[ceil(pcells / 32)].
__global__ __launch_bounds__(AS_THREADS) void nav_field_kernel(ExpertGrid g, const uint32_t* __restrict__ bitmap,
                                                               const double* __restrict__ state, uint32_t* __restrict__ field,
                                                               long long* __restrict__ tag) {
  extern __shared__ uint32_t as_lds[];
  uint32_t* dist = as_lds;                  // [pcells], padded (iy + 1) * pw + ix + 1
  uint32_t* occ = as_lds + g.pcells;        // [ceil(pcells / 32)] bits, same index
  __shared__ int s_flag[3];                 // what a sweep found, rotating so that one barrier per sweep is enough
  __shared__ int s_goal[2];                 // padded index of the goal cell (-1: nothing to do), iy * w + ix of it

  const int tid = threadIdx.x;
  const long long i = blockIdx.x;
  if (tid == 0) {
    s_flag[0] = s_flag[1] = s_flag[2] = 0;
    int ix = 0, iy = 0, gidx = -1, cell = 0;
    if (ex_cell(g, state[NAV_STATE * i + 3], state[NAV_STATE * i + 4], &ix, &iy) == EX_OK) {
      const int p = (iy + 1) * g.pw + ix + 1;
      cell = iy * g.w + ix;
      if (!ex_bit(bitmap, p) && tag[i] != (long long)cell + 1) gidx = p;
    }
    s_goal[0] = gidx;
    s_goal[1] = cell;
  }
  __syncthreads();
  const int gidx = s_goal[0];
  if (gidx < 0) return;                                        // uniform: no valid goal, or the cached field is this goal's

  const int occ_words = (g.pcells + 31) >> 5;
  for (int k = tid; k < occ_words; k += AS_THREADS) occ[k] = bitmap[k];
  for (int k = tid; k < g.pcells; k += AS_THREADS) dist[k] = AS_UNREACHED;
  __syncthreads();

  // cells tid, tid + 1024, ... of the padded array are this thread's; bit k of `own`: cell k is interior, unblocked and
  // not the goal, which holds (0, 0) for good
  uint64_t own = 0;
  for (int k = 0, idx = tid; idx < g.pcells; ++k, idx += AS_THREADS) {
    const int px = idx % g.pw, py = idx / g.pw;
    const bool interior = px >= 1 && px <= g.w && py >= 1 && py <= g.h;
    if (interior && !ex_bit(occ, idx) && idx != gidx) own |= uint64_t(1) << k;
  }
  if (tid == 0) dist[gidx] = 0u;
  __syncthreads();

  // to the fixpoint: the robot moves, so every cell's pair is needed; a sweep that changes something settles at least
  // one more cell, hence the bound of w * h sweeps
  int sweep = 0;
  bool converged = false;
  while (sweep < g.max_sweeps) {
    const bool changed = ex_sweep(dist, own, tid, g.pw);
    if (tid == 0) s_flag[(sweep + 1) % 3] = 0;                 // its last readers passed the previous barrier
    if (changed) atomicOr(&s_flag[sweep % 3], 1);
    __syncthreads();
    const int flag = s_flag[sweep % 3];
    ++sweep;
    if (!flag) { converged = true; break; }
  }
  if (!converged) {                                            // uniform
    if (tid == 0) tag[i] = -1;
    return;
  }
  uint32_t* out = field + i * (long long)g.pcells;
  for (int k = tid; k < g.pcells; k += AS_THREADS) out[k] = dist[k];
  __syncthreads();
  if (tid == 0) tag[i] = (long long)s_goal[1] + 1;             // last
}

// ---- porl_nav_expert, second launch: waypoint, path, command ----------------------------------------------------------------
struct ExpertSteerArgs {
  const double* state; const long long* tag; const uint32_t* field; const uint32_t* bitmap;
  long long n;
  int lookahead, max_path, n_actions;
  double dt, max_lin_vel, max_ang_vel, ang_step;
  float* commands; long long cmd_stride;       // (n, 2) v, w
  float* scores; long long score_stride;       // (n, n_actions)
  double* waypoint; int32_t* path_len; int32_t* status; int32_t* path;
};

// One thread per robot.
__global__ __launch_bounds__(EX_STEER_THREADS) void nav_steer_kernel(ExpertGrid g, ExpertSteerArgs a) {
  NAV_EXACT
  const long long i = (long long)blockIdx.x * EX_STEER_THREADS + threadIdx.x;
  if (i >= a.n) return;
  const double* st = a.state + NAV_STATE * i;
  const double x = st[0], y = st[1], yaw = st[2], gx = st[3], gy = st[4];
  const uint32_t* f = a.field + i * (long long)g.pcells;
  int32_t* path = a.path ? a.path + i * 2 * (long long)a.max_path : nullptr;
  const int pw = g.pw;
  double wx = gx, wy = gy;                                     // every status but EX_OK steers straight at the goal
  int status = EX_OK, n_nodes = 0, written = 0;
  int gix = 0, giy = 0, rix = 0, riy = 0;

  if (!isfinite(x) || !isfinite(y) || !isfinite(yaw)) status = EX_NON_FINITE;
  if (status == EX_OK) status = ex_cell(g, gx, gy, &gix, &giy);
  const int gidx = (giy + 1) * pw + gix + 1;
  if (status == EX_OK && ex_bit(a.bitmap, gidx)) status = EX_GOAL_BLOCKED;
  if (status == EX_OK && a.tag[i] != (long long)(giy * g.w + gix) + 1) status = EX_NOT_CONVERGED;
  if (status == EX_OK) {
    const int rs = ex_cell(g, x, y, &rix, &riy);
    if (rs != EX_OK) status = rs == EX_NON_FINITE ? EX_NON_FINITE : EX_NO_FIELD;
  }
  if (status == EX_OK) {
    int cur = (riy + 1) * pw + rix + 1, steps = 0;
    uint32_t vc = f[cur];
    if (vc == AS_UNREACHED) {                                  // start from the reached neighbour of least cost: the first step
      double cb = 0.0;
      int nb = -1;
      for (int k = 0; k < 8; ++k) {
        const int n = cur + ex_dy(k) * pw + ex_dx(k);
        const uint32_t v = f[n];
        if (v == AS_UNREACHED) continue;
        const double c = as_cost(v);
        if (nb < 0 || c < cb) { cb = c; nb = n; vc = v; }
      }
      if (nb < 0) {
        status = EX_NO_FIELD;
      } else {                                                 // the path still begins at the robot's own cell
        if (path && written < a.max_path) { path[2 * written] = rix; path[2 * written + 1] = riy; ++written; }
        cur = nb;
        steps = 1;
      }
    }
    if (status == EX_OK) {
      const int left = (int)(vc >> 16) + (int)(vc & 0xFFFFu);   // moves from `cur` to the goal
      n_nodes = left + 1 + steps;
      if (path && written < a.max_path) { path[2 * written] = cur % pw - 1; path[2 * written + 1] = cur / pw - 1; ++written; }
      bool have = false;
      for (int m = 0; m <= left; ++m) {
        if (!have && (cur == gidx || steps >= a.lookahead)) {
          have = true;
          if (cur != gidx) { wx = (double)(cur % pw - 1) * g.res + g.min_x; wy = (double)(cur / pw - 1) * g.res + g.min_y; }
          if (!path) break;
        }
        if (cur == gidx) break;
        int nx = -1;
        uint32_t vn = 0;
        for (int k = 0; k < 8 && nx < 0; ++k) {
          const int n = cur + ex_dy(k) * pw + ex_dx(k);
          const uint32_t v = f[n];
          if (v != AS_UNREACHED && v + (k < 4 ? 0x10000u : 1u) == vc) { nx = n; vn = v; }
        }
        if (nx < 0) break;                                     // not at a fixpoint: cannot happen behind a converged field
        cur = nx; vc = vn; ++steps;
        if (path && written < a.max_path) { path[2 * written] = cur % pw - 1; path[2 * written + 1] = cur / pw - 1; ++written; }
      }
    }
  }
  if (status != EX_OK) { n_nodes = 0; written = 0; }
  if (path) for (int k = written; k < a.max_path; ++k) { path[2 * k] = -1; path[2 * k + 1] = -1; }
  if (a.waypoint) { a.waypoint[2 * i] = wx; a.waypoint[2 * i + 1] = wy; }
  if (a.path_len) a.path_len[i] = n_nodes;
  if (a.status) a.status[i] = status;

  // the command: heading error to the waypoint, wrapped as navd_tail wraps
  const double PI = 3.141592653589793;
  double e = atan2(wy - y, wx - x) - yaw;
  if (e > PI) e -= 2.0 * PI;
  else if (e < -PI) e += 2.0 * PI;
  const bool live = status != EX_NON_FINITE;                   // a non-finite pose or goal: the zero command, zero scores
  if (a.commands) {
    double om = e / a.dt;
    om = om < -a.max_ang_vel ? -a.max_ang_vel : (om > a.max_ang_vel ? a.max_ang_vel : om);
    const double c = cos(e);
    const double v = a.max_lin_vel * (c > 0.0 ? c : 0.0);
    a.commands[i * a.cmd_stride] = live ? (float)v : 0.f;
    a.commands[i * a.cmd_stride + 1] = live ? (float)om : 0.f;
  }
  if (a.scores) {
    for (int k = 0; k < a.n_actions; ++k) {
      const double wa = ((double)(a.n_actions - 1) / 2.0 - (double)k) * a.ang_step;
      a.scores[i * a.score_stride + k] = live ? (float)(-fabs(e - wa * a.dt)) : 0.f;
    }
  }
}

}  // namespace porl
