"""An A* expert for the lidar navigation task, planned on the device (csrc/expert.hpp): the reference's
dataloader/a_star.py `AStarPlanner.planning` for every robot of a simulator per call, with no read-back.

    sim = LidarNavSim(NavWorld.lattice(), n_envs=1024, auto_reset=True)
    expert = AStarExpert(sim)                             # rasterises the simulator's own world once
    rows, timeouts = collect(sim, act=expert, n_steps=200)
    waypoint, path_len, status, path = expert.plan(max_path=64)

`PlanGrid` is the occupancy grid of a world: a cell is blocked iff its centre lies within `inflate` of a wall segment or a
pillar.  `AStarExpert` keeps one exact 8-connected distance field per robot, grown from the robot's goal cell and
refreshed only when that cell changes, descends it `lookahead` cells to a waypoint and steers at the waypoint: a command
`v, w` for a LidarNavSim, a table of action scores for a DiscreteLidarNavSim (`engine.qnet_select` on it picks the
nearest turn).  Rules, tie-breaking and the deviations from the reference planner: DESIGN.md §4t.

The expert is PRIVILEGED: it reads the robots' poses and goals from `sim.state` and the world itself, not the
observation.  There is no CPU path: CPU tensors raise `NativeError`.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from .. import _native as N
from .navsim import _need_cuda

STATUS_NAMES = ("ok", "no_field", "goal_off_grid", "goal_blocked", "non_finite", "not_converged")
OK, NO_FIELD, GOAL_OFF_GRID, GOAL_BLOCKED, NON_FINITE, NOT_CONVERGED = range(6)
MAX_PADDED_CELLS, MAX_LDS_BYTES, MAX_PAIR = 65536, 160 * 1024 - 1024, 65534
UNREACHED = 0xFFFFFFFF

Plan = namedtuple("Plan", "waypoint path_len status path")


class PlanGrid:
    """The occupancy grid of `world`: `w x h` cells of `resolution`, the centre of cell (ix, iy) at `ix * resolution +
    min_x, iy * resolution + min_y`.  For a world with an `origin` the defaults are `min = origin` and `w = h = round(cells
    / resolution) + 1`, so cell centres lie on both walls.  The bitmap is built once, here, on the world's device
    (`device`: move the world there first)."""

    def __init__(self, world, resolution=0.1, inflate=0.18, min_x=None, min_y=None, w=None, h=None, cells=5, device=None):
        if device is not None:
            world = world.to(device)
        if (min_x is None or min_y is None) and world.origin is None:
            raise ValueError("a custom world has no origin: pass min_x and min_y")
        _need_cuda(world.segments, world.circles)
        if not resolution > 0:
            raise ValueError("resolution must be positive")
        if not inflate >= 0:
            raise ValueError("inflate must not be negative")
        self.world = world
        self.resolution, self.inflate = float(resolution), float(inflate)
        self.min_x = float(world.origin[0] if min_x is None else min_x)
        self.min_y = float(world.origin[1] if min_y is None else min_y)
        side = round(cells / resolution) + 1
        self.w, self.h = int(side if w is None else w), int(side if h is None else h)
        if self.w < 1 or self.h < 1:
            raise ValueError("w and h must be positive")
        self.pw, self.pcells = self.w + 2, (self.w + 2) * (self.h + 2)
        n_words = (self.pcells + 31) // 32
        if self.pcells > MAX_PADDED_CELLS or 4 * (self.pcells + n_words) > MAX_LDS_BYTES or self.w + self.h > MAX_PAIR:
            raise ValueError(f"a {self.w} x {self.h} grid does not fit one workgroup: {self.pcells} padded cells (at most "
                             f"{MAX_PADDED_CELLS}), {4 * (self.pcells + n_words)} bytes of LDS (at most {MAX_LDS_BYTES})")
        self._c = N.NavGrid(self.resolution, self.inflate, self.min_x, self.min_y, self.w, self.h)
        self.bitmap = torch.zeros(n_words, dtype=torch.int32, device=world.device)
        seg, cir = world.segments, world.circles
        N.check(N.lib().porl_nav_rasterize(N.ptr(seg), seg.shape[0], N.ptr(cir), cir.shape[0], self._c, N.ptr(self.bitmap),
                                           n_words, N.current_stream_ptr(self.bitmap)), "porl_nav_rasterize")

    @property
    def device(self):
        return self.bitmap.device

    def interior(self, padded):
        """(..., w, h) view `[ix, iy]` of the interior of a (..., pcells) array in the padded layout."""
        lead = padded.shape[:-1]
        return padded.reshape(*lead, self.h + 2, self.pw)[..., 1:-1, 1:-1].transpose(-1, -2)

    def occupancy(self):
        """(w, h) bool on the device: `[ix, iy]` is True where the cell is blocked."""
        p = torch.arange(self.pcells, device=self.device)
        bits = (self.bitmap.to(torch.int64)[p >> 5] >> (p & 31)) & 1
        return self.interior(bits.bool()).contiguous()


class AStarExpert:
    """The planner and driver of `sim`, a LidarNavSim or a DiscreteLidarNavSim, on `grid` (default: `PlanGrid(sim.world)`).
    Owns the cache: `fields` (N, padded cells) and `tags` (N,) int64, tag[i] = iy * w + ix + 1 of the goal cell whose
    field row i holds, 0 for none.  `N * padded cells * 4` bytes may not exceed `max_cache_bytes` (ValueError)."""

    def __init__(self, sim, grid=None, lookahead=2, max_cache_bytes=1 << 30):
        if int(lookahead) < 1:
            raise ValueError("lookahead must be at least 1")
        self.sim = sim
        self.grid = PlanGrid(sim.world) if grid is None else grid
        if self.grid.device != sim.state.device:
            raise ValueError(f"the grid lives on {self.grid.device}, the simulator on {sim.state.device}")
        self.lookahead = int(lookahead)
        self.discrete = hasattr(sim, "n_actions")
        n, need = sim.n_envs, sim.n_envs * self.grid.pcells * 4
        if need > max_cache_bytes:
            raise ValueError(f"the field cache of {n} robots x {self.grid.pcells} padded cells is {need} bytes, more than "
                             f"max_cache_bytes = {max_cache_bytes}")
        dev = sim.state.device
        self.fields = torch.zeros(n, self.grid.pcells, dtype=torch.int32, device=dev)
        self.tags = torch.zeros(n, dtype=torch.int64, device=dev)
        p = sim.params
        self.n_actions = sim.n_actions if self.discrete else 0
        self._ang_step = p["max_ang_vel"] * 0.5 if self.discrete else 0.0

    def _launch(self, commands=None, scores=None, waypoint=None, path_len=None, status=None, path=None, max_path=0):
        sim, p = self.sim, self.sim.params
        cp = N.NavExpertParams(p["dt"], p["max_lin_vel"], p["max_ang_vel"], self._ang_step, self.n_actions, self.lookahead,
                               int(max_path), 0)
        N.check(N.lib().porl_nav_expert(self.grid._c, N.ptr(self.grid.bitmap), cp, N.ptr(sim.state), N.ptr(self.fields),
                                        N.ptr(self.tags), N.ptr(commands), 0 if commands is None else commands.stride(0),
                                        N.ptr(scores), 0 if scores is None else max(scores.stride(0), scores.shape[1]),
                                        N.ptr(waypoint), N.ptr(path_len), N.ptr(status), N.ptr(path), sim.n_envs,
                                        N.current_stream_ptr(sim.state)), "porl_nav_expert")

    def __call__(self, obs=None, out=None):
        """Act for every robot from `sim.state` — `obs` is accepted and ignored: the expert is privileged.  Returns (N, 2)
        fp32 commands `v, w` for a LidarNavSim (what `collect(sim, act=expert)` and `evaluate_policy_batched(expert, sim,
        ...)` take), (N, A) fp32 action scores for a DiscreteLidarNavSim.  `out`: a contiguous fp32 tensor of that shape to
        write into."""
        n = self.sim.n_envs
        shape = (n, self.n_actions) if self.discrete else (n, 2)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.sim.state.device)
        else:
            _need_cuda(out)
            if out.shape != shape or out.dtype != torch.float32 or not out.is_contiguous():
                raise ValueError(f"out: expected a contiguous {shape} float32 tensor")
        if self.discrete:
            self._launch(scores=out)
        else:
            self._launch(commands=out)
        return out

    def plan(self, max_path=0):
        """The device form of `AStarPlanner.planning`: Plan(waypoint (N, 2) fp64, path_len (N,) int32 — nodes from the
        robot's cell to the goal's, both included, 0 without a path —, status (N,) int32 (STATUS_NAMES), path (N, max_path,
        2) int32 cells `ix, iy` from the robot's to the goal's, truncated at max_path, the rest -1; None for max_path 0)."""
        if max_path < 0:
            raise ValueError("max_path must not be negative")
        n, dev = self.sim.n_envs, self.sim.state.device
        waypoint = torch.empty(n, 2, dtype=torch.float64, device=dev)
        path_len = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        path = torch.empty(n, max_path, 2, dtype=torch.int32, device=dev) if max_path else None
        self._launch(waypoint=waypoint, path_len=path_len, status=status, path=path, max_path=max_path)
        return Plan(waypoint, path_len, status, path)

    def field(self, i):
        """The cached field of robot i as two (w, h) int32 tensors `(a, b)` indexed `[ix, iy]`: axis and diagonal moves of
        a cheapest path to the goal cell, -1 where unreached."""
        v = self.grid.interior(self.fields[i].to(torch.int64) & UNREACHED)
        un = v == UNREACHED
        a = torch.where(un, torch.full_like(v, -1), v >> 16).to(torch.int32)
        b = torch.where(un, torch.full_like(v, -1), v & 0xFFFF).to(torch.int32)
        return a.contiguous(), b.contiguous()

    def invalidate(self):
        """Forget every cached field (the next call relaxes every robot)."""
        self.tags.zero_()
