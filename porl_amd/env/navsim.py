"""The lidar navigation task of the reference's env/gazebo.py on the device, without ROS and Gazebo (csrc/navsim.hpp).

A unicycle step over `dt` and a 2-D ray cast against wall segments and pillars replace the physics and the laser; the
observation, the shaped reward, the termination rules and the start / goal draw are env/gazebo.py's.  One launch steps
every robot of a simulator.

    world = NavWorld.lattice()                          # the 5 m x 5 m square random_pts_map draws in
    sim = LidarNavSim(world, n_envs=4096, seed=0)
    obs = sim.reset()
    out = sim.step(actions)                             # NavStep(next_obs, reward, terminated, truncated, status)
    rows, timeouts = collect(sim_auto_reset, None, 200) # transition rows for PackedReplay / label_dataset

What this is not: no inertia, no collision response, no sensor noise; the scan is taken at the pose the
step reaches.  `reset` does not test a spawn point against the world, as the reference does not: a custom world must keep
the interiors `k + [spawn_lo, spawn_lo + spawn_span]` of its cells free.

There is no CPU path: CPU tensors raise `NativeError`.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .. import _native as N

# env/gazebo.py's constants (:32-33, :48-53, :105-131, :280-318) and what lidarPreprocess (:77-83) makes of inf
DEFAULTS = dict(dt=0.2, max_lin_vel=0.15, max_ang_vel=1.5, min_range=0.13, range_max=3.5, no_return=10.0, goal_radius=0.2,
                hit_reward=-500.0, goal_reward=500.0, origin_x=None, origin_y=None, spawn_lo=0.16, spawn_span=0.68,
                min_gap_sq=0.01, goal_dist_lo=0.3, goal_dist_hi=3.5, n_beams=360, episode_step=500, cells=5)
STATUS_NAMES = ("running", "hit", "goal", "timelimited")
RUNNING, HIT, GOAL, TIMELIMITED, DRAW_CAP = 0, 1, 2, 3, 256
LAYOUTS = {"goal": 0, "pose": 1}
MAX_PRIMS, MAX_BEAMS = 2048, 1024

NavStep = namedtuple("NavStep", "next_obs reward terminated truncated status")


def beam_table(n_beams):
    """(n_beams, 2) fp64 cos / sin of the beams' angles in the robot frame, by scalar numpy calls: `i * pi / 180` for the
    reference's 360 beams (the convention of dataloader/astar.py), `2 pi i / n` otherwise."""
    if n_beams == 360:
        ang = [i * np.pi / 180 for i in range(360)]
    else:
        ang = [2 * np.pi * i / n_beams for i in range(n_beams)]
    return np.array([[np.cos(a), np.sin(a)] for a in ang], dtype=np.float64)


class NavWorld:
    """Wall segments (M, 4) `x1 y1 x2 y2` and solid pillars (C, 3) `cx cy r`, fp32, shared by all robots of a simulator.
    `origin` is where `random_pts_map` places its 5 x 5 cells (None for a custom world: pass origin_x / origin_y to the
    simulator)."""

    def __init__(self, segments, circles=None, origin=None):
        seg = torch.as_tensor(segments, dtype=torch.float32).reshape(-1, 4).contiguous()
        cir = torch.as_tensor(circles if circles is not None else np.zeros((0, 3)), dtype=torch.float32).reshape(-1, 3).contiguous()
        if seg.shape[0] + cir.shape[0] > MAX_PRIMS:
            raise ValueError(f"{seg.shape[0]} segments + {cir.shape[0]} circles: at most {MAX_PRIMS} primitives")
        if seg.device != cir.device:
            raise ValueError("segments and circles live on different devices")
        self.segments, self.circles, self.origin = seg, cir, origin

    @classmethod
    def lattice(cls, rank=0, pillar_radius=0.08, map_x=-10., map_y=-10., cells=5):
        """The default world: the square `random_pts_map` draws in for process `rank` (env/gazebo.py:298-302), four walls
        and a pillar on every interior lattice point.  With pillar_radius <= 0.096 every spawn point of the reference's
        rule reads min(scan) >= 0.13."""
        ox, oy = map_x + (rank % 4) * cells, map_y + (3 - rank // 4) * cells
        L = float(cells)
        seg = [[ox, oy, ox + L, oy], [ox + L, oy, ox + L, oy + L], [ox + L, oy + L, ox, oy + L], [ox, oy + L, ox, oy]]
        cir = [[ox + i, oy + j, pillar_radius] for j in range(1, cells) for i in range(1, cells)]
        return cls(np.array(seg, np.float32), np.array(cir, np.float32).reshape(-1, 3), origin=(float(ox), float(oy)))

    def to(self, device):
        return NavWorld(self.segments.to(device), self.circles.to(device), self.origin)

    @property
    def device(self):
        return self.segments.device


def _need_cuda(*tensors):
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise N.NativeError(f"the navigation simulator runs on a HIP device only (tensor on {t.device}); no CPU path")


def _rows_stride(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def nav_scan(segments, circles, poses, n_beams=360, range_max=3.5, no_return=10.0, out=None):
    """The ray cast alone (porl_nav_scan): ranges (n, n_beams) fp32 from `poses` (n, 3) fp64 `x y yaw`."""
    if not 1 <= n_beams <= MAX_BEAMS:
        raise ValueError(f"n_beams {n_beams} outside [1, {MAX_BEAMS}]")
    _need_cuda(segments, circles, poses, out)
    if poses.dim() != 2 or poses.shape[1] != 3 or poses.dtype != torch.float64:
        raise ValueError(f"poses: expected (n, 3) float64, got {poses.dtype} {tuple(poses.shape)}")
    if segments.dtype != torch.float32 or circles.dtype != torch.float32:
        raise ValueError("segments and circles must be float32")
    segments, circles, poses = segments.reshape(-1, 4).contiguous(), circles.reshape(-1, 3).contiguous(), poses.contiguous()
    n = poses.shape[0]
    if out is None:
        out = torch.empty(n, n_beams, dtype=torch.float32, device=poses.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape != (n, n_beams) or (n_beams > 1 and out.stride(1) != 1):
        raise ValueError("out: expected (n, n_beams) float32 with unit column stride")
    if n == 0:
        return out
    dirs = _dirs(n_beams, poses.device)
    p = N.NavParams(range_max=range_max, no_return=no_return, n_beams=n_beams)
    N.check(N.lib().porl_nav_scan(N.ptr(segments), segments.shape[0], N.ptr(circles), circles.shape[0], N.ptr(poses), N.ptr(dirs),
                                  p, N.ptr(out), _rows_stride(out), n, N.current_stream_ptr(poses)), "porl_nav_scan")
    return out


_dir_cache: dict = {}


def _dirs(n_beams, device):
    key = (str(device), n_beams)
    if key not in _dir_cache:
        _dir_cache[key] = torch.from_numpy(beam_table(n_beams)).to(device)
    return _dir_cache[key]


class LidarNavSim:
    """`n_envs` robots in one world.  Robot i draws its starts and goals from the stream keyed by (seed, env_offset + i), so
    one simulator of 64 equals two of 32 with env_offset 0 and 32.  Keyword parameters: DEFAULTS (origin_x / origin_y
    default to the world's origin).

    state (N, 8) fp64 `x y yaw goal_x goal_y prev_goal_distance prev_goal_angle 0`, counters (N, 4) int64 `n_step episode
    status draws_used`; status 0 running, 1 hit, 2 goal, 3 timelimited, bit 8 (256) = a reset stopped at 256 draws."""

    def __init__(self, world, n_envs, seed=0, env_offset=0, layout="goal", auto_reset=False, device="cuda", **params):
        unknown = set(params) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"unknown parameter(s) {sorted(unknown)}; known: {sorted(DEFAULTS)}")
        if layout not in LAYOUTS:
            raise ValueError(f"layout {layout!r}: one of {sorted(LAYOUTS)}")
        if n_envs < 1:
            raise ValueError("n_envs must be positive")
        p = dict(DEFAULTS)
        p.update(params)
        for k, o in (("origin_x", 0), ("origin_y", 1)):
            if p[k] is None:
                if world.origin is None:
                    raise ValueError(f"a custom world has no origin: pass {k}")
                p[k] = world.origin[o]
        if not p["max_lin_vel"] * p["dt"] < p["min_range"]:
            raise ValueError("max_lin_vel * dt must stay below min_range: a robot could pass a wall between two scans")
        if not p["max_ang_vel"] * p["dt"] < np.pi:
            raise ValueError("max_ang_vel * dt must stay below pi: the heading is wrapped by one turn per step")
        if not 1 <= p["n_beams"] <= MAX_BEAMS:
            raise ValueError(f"n_beams {p['n_beams']} outside [1, {MAX_BEAMS}]")
        device = torch.device(device)
        if device.type != "cuda":
            raise N.NativeError(f"the navigation simulator runs on a HIP device only (device {device}); no CPU path")
        self.world = world.to(device)
        self.params, self.layout, self.auto_reset = p, layout, bool(auto_reset)
        self.n_envs, self.seed, self.env_offset, self.device = int(n_envs), int(seed) & (2 ** 64 - 1), int(env_offset), device
        self.n_beams = int(p["n_beams"])
        self.obs_dim = self.n_beams + (5 if layout == "pose" else 2)
        self.row_width = 2 * self.obs_dim + 4
        self._cp = N.NavParams(**{k: p[k] for k in DEFAULTS}, layout=LAYOUTS[layout], auto_reset=int(self.auto_reset))
        self._dirs = _dirs(self.n_beams, device)
        n, S = self.n_envs, self.obs_dim
        self.state = torch.zeros(n, 8, dtype=torch.float64, device=device)
        self.counters = torch.zeros(n, 4, dtype=torch.int64, device=device)
        self.counters[:, 2] = TIMELIMITED                 # nothing runs before the first reset
        self.obs = torch.zeros(n, S, dtype=torch.float32, device=device)

    def _world_args(self):
        w = self.world
        return N.ptr(w.segments), w.segments.shape[0], N.ptr(w.circles), w.circles.shape[0], N.ptr(self._dirs), self._cp

    def reset(self, mask=None):
        """Reset all robots, or those where `mask` (N,) is set: episode += 1, a new start and goal.  Returns `obs`."""
        m = None
        if mask is not None:
            _need_cuda(mask)
            if mask.shape != (self.n_envs,):
                raise ValueError(f"mask: expected ({self.n_envs},), got {tuple(mask.shape)}")
            m = mask.to(torch.uint8).contiguous()
        N.check(N.lib().porl_nav_reset(*self._world_args(), self.seed, self.env_offset, N.ptr(m), N.ptr(self.state),
                                       N.ptr(self.counters), N.ptr(self.obs), self.obs.stride(0), self.n_envs,
                                       N.current_stream_ptr(self.state)), "porl_nav_reset")
        return self.obs

    def step(self, actions, rows=None):
        """One step of every running robot with commands `actions` (N, 2) fp32 `v [m/s], w [rad/s]` (clipped to the
        robot's limits; non-finite counts as 0).  `rows`: an optional (N, 2S + 4) fp32 view with unit column stride that
        receives `[s | r | s' | terminated | v w]`; any row stride, so `store.view(N, T, W)[:, t]` fills an env-major
        store.  Returns NavStep; `sim.obs` is what to act on next."""
        _need_cuda(actions, rows)
        n, S = self.n_envs, self.obs_dim
        if actions.shape != (n, 2) or actions.dtype != torch.float32:
            raise ValueError(f"actions: expected ({n}, 2) float32, got {actions.dtype} {tuple(actions.shape)}")
        if actions.stride(1) != 1:
            actions = actions.contiguous()
        if rows is not None:
            if rows.shape != (n, self.row_width) or rows.dtype != torch.float32 or rows.stride(1) != 1:
                raise ValueError(f"rows: expected ({n}, {self.row_width}) float32 with unit column stride")
        dev = self.device
        next_obs = torch.empty(n, S, dtype=torch.float32, device=dev)
        reward = torch.empty(n, dtype=torch.float32, device=dev)
        flags = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        N.check(N.lib().porl_nav_step(*self._world_args(), self.seed, self.env_offset, N.ptr(actions), _rows_stride(actions),
                                      N.ptr(self.state), N.ptr(self.counters), N.ptr(self.obs), self.obs.stride(0),
                                      N.ptr(next_obs), S, N.ptr(reward), N.ptr(flags), N.ptr(status), N.ptr(rows),
                                      0 if rows is None else _rows_stride(rows), n, N.current_stream_ptr(self.state)),
                "porl_nav_step")
        return NavStep(next_obs, reward, (flags & 1).bool(), (flags & 2).bool(), status)

    def set_state(self, state=None, counters=None, obs=None):
        """Overwrite the resident state / counters / observation (tests and restarts); `prev_*` are the caller's."""
        for dst, src in ((self.state, state), (self.counters, counters), (self.obs, obs)):
            if src is not None:
                dst.copy_(torch.as_tensor(src).to(dst.device, dst.dtype).reshape(dst.shape))

    def scan(self, poses):
        """Ranges (n, n_beams) fp32 from `poses` (n, 3) fp64 in this simulator's world."""
        return nav_scan(self.world.segments, self.world.circles, poses, n_beams=self.n_beams,
                        range_max=self.params["range_max"], no_return=self.params["no_return"])


_command_consts: dict = {}


def random_command(n, generator=None, device="cuda"):
    """collect.py:38's uniform random command, `(u * 2 + [0, -1]) * [0.075, 1.5]`, for n robots (the two constants are
    uploaded once per device)."""
    device = torch.device(device)
    if device not in _command_consts:
        _command_consts[device] = (torch.tensor([0., -1.], device=device), torch.tensor([0.15 / 2, 1.5], device=device))
    shift, scale = _command_consts[device]
    return (torch.rand(n, 2, generator=generator, device=device, dtype=torch.float32) * 2 + shift) * scale


def collect(sim, act=None, n_steps=100, layout=None, generator=None):
    """Roll `sim` (auto_reset=True) for `n_steps` and return (rows (N * T, 2S + 4), timeouts (N * T,) fp32 0 / 1): an env-major
    store — robot i's trajectory is rows[i * T:(i + 1) * T] — in the layout `PackedReplay` reads, `[s | r | s' | done |
    a]`, and the flags that close an episode: the steps that terminated or hit the step limit, and each robot's last
    collected step (the store cuts that episode), so `EpisodeIndex.from_replay(rows, timeouts=timeouts)` delimits exactly
    the simulator's episodes and never joins two robots.  `act`: obs -> (N, 2) device commands; default collect.py:38's
    uniform random command under `generator`."""
    if not sim.auto_reset:
        raise ValueError("collect needs a simulator with auto_reset=True")
    if layout is not None and layout != sim.layout:
        raise ValueError(f"the simulator observes in layout {sim.layout!r}, not {layout!r}")
    if n_steps < 1:
        raise ValueError("n_steps must be positive")
    n, T, W = sim.n_envs, int(n_steps), sim.row_width
    store = torch.empty(n * T, W, dtype=torch.float32, device=sim.device)
    timeouts = torch.zeros(n, T, dtype=torch.bool, device=sim.device)
    view = store.view(n, T, W)
    if bool((sim.counters[:, 2] & 0xff != RUNNING).any()):
        sim.reset()
    for t in range(T):
        a = random_command(n, generator, sim.device) if act is None else act(sim.obs)
        out = sim.step(a.to(torch.float32), rows=view[:, t])
        timeouts[:, t] = out.truncated | out.terminated
    timeouts[:, T - 1] = True
    return store, timeouts.reshape(-1).to(torch.float32)
