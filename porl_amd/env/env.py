"""The reference's env/env.py — the 5-action TurtleBot task runner.py hands to DQN_CQL — on the device, without ROS and
Gazebo (csrc/navsim_discrete.hpp): the world, ray cast, unicycle step and start / goal draw of env/navsim.py under the
discrete task's rules.

    sim = DiscreteLidarNavSim(NavWorld.lattice(), n_envs=1024, auto_reset=True)
    sim.reset()
    out = sim.step(actions, replay=DeviceReplay(100000, sim.obs_dim))   # NavStep; the transitions land in the replay
    env = Env(5, 362)                                                   # the reference's class on one robot

Rules (line numbers of env/env.py): the robot drives at `lin_vel` = 0.15 m/s and action a of A picks the angular velocity
((A - 1) / 2 - a) * max_ang_vel * 0.5 (:139-144); the observation is [scan | heading | distance], heading and distance
rounded to two decimals (:59-75, :96-102), a beam without return reads 3.5 (:84-85); a hit is 0 < min(scan) < min_range,
the goal is a rounded distance < 0.2, and the goal wins (:92-99, :123-134); the reward is a yaw term times 2 ** (distance /
goal_distance), or +-200 (:104-136); `truncated` at `episode_step` = 500 steps, status `timelimited` then, reward unchanged
(:160-164); reset draws as random_pts_map with a goal 0.25 .. 3.5 away (:270-308).

An action index outside [0, A) that reaches the kernel is clamped into range (the reference raises IndexError on its yaw
table, or drives an angular velocity off the table).  `round(x, 2)` is restated as rint(100 x) / 100 in fp64.
No ROS wait, no simulator pause.  There is no CPU path: CPU tensors raise `NativeError`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _native as N
from .navsim import DEFAULTS as _NAV_DEFAULTS
from .navsim import MAX_BEAMS, STATUS_NAMES, TIMELIMITED, NavStep, NavWorld, _dirs, _need_cuda

# env/env.py's constants: porl_nav_params' geometry, limits and reset constants (:48-50, :84-85, :97, :270-308) and the
# task's own (:139-143, :126, :132)
DEFAULTS = dict(_NAV_DEFAULTS, no_return=3.5, goal_dist_lo=0.25, hit_reward=-200.0, goal_reward=200.0, lin_vel=None)
MAX_ACTIONS = 5


class DiscreteLidarNavSim:
    """`n_envs` robots of the discrete task in one world.  Robot i draws its starts and goals from the stream keyed by
    (seed, env_offset + i).  Keyword parameters: DEFAULTS (`lin_vel` defaults to `max_lin_vel`, origin_x / origin_y to the
    world's origin).  `n_actions` must lie in [1, 5]: the reference's yaw table has five entries.

    state (N, 8) fp64 `x y yaw goal_x goal_y 0 0 goal_distance`, counters (N, 4) int64 `n_step episode status draws_used`
    (status as LidarNavSim's), tallies (N, 4) fp64 `episodes, sum of returns, goals, hits` added to at every episode's end
    (the host reads them whenever it likes), obs (N, n_beams + 2) fp32 `[scan | heading | distance]`."""

    def __init__(self, world, n_envs, n_actions=5, seed=0, env_offset=0, auto_reset=False, device="cuda", **params):
        unknown = set(params) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"unknown parameter(s) {sorted(unknown)}; known: {sorted(DEFAULTS)}")
        if not 1 <= int(n_actions) <= MAX_ACTIONS:
            raise ValueError(f"n_actions {n_actions} outside [1, {MAX_ACTIONS}]: the reference's yaw table has five entries")
        if n_envs < 1:
            raise ValueError("n_envs must be positive")
        p = dict(DEFAULTS)
        p.update(params)
        if p["lin_vel"] is None:
            p["lin_vel"] = p["max_lin_vel"]
        for k, o in (("origin_x", 0), ("origin_y", 1)):
            if p[k] is None:
                if world.origin is None:
                    raise ValueError(f"a custom world has no origin: pass {k}")
                p[k] = world.origin[o]
        ang_step = p["max_ang_vel"] * 0.5
        if not max(p["lin_vel"], p["max_lin_vel"]) * p["dt"] < p["min_range"]:
            raise ValueError("lin_vel * dt must stay below min_range: a robot could pass a wall between two scans")
        if not p["max_ang_vel"] * p["dt"] < np.pi:
            raise ValueError("max_ang_vel * dt must stay below pi: the heading is wrapped by one turn per step")
        if not 1 <= p["n_beams"] <= MAX_BEAMS:
            raise ValueError(f"n_beams {p['n_beams']} outside [1, {MAX_BEAMS}]")
        device = torch.device(device)
        if device.type != "cuda":
            raise N.NativeError(f"the navigation simulator runs on a HIP device only (device {device}); no CPU path")
        self.world = world.to(device)
        self.params, self.auto_reset, self.n_actions = p, bool(auto_reset), int(n_actions)
        self.n_envs, self.seed, self.env_offset, self.device = int(n_envs), int(seed) & (2 ** 64 - 1), int(env_offset), device
        self.n_beams = int(p["n_beams"])
        self.obs_dim = self.n_beams + 2
        self._cp = N.NavParams(**{k: p[k] for k in _NAV_DEFAULTS}, layout=0, auto_reset=int(self.auto_reset))
        self._task = N.NavDiscrete(self.n_actions, p["lin_vel"], ang_step, p["goal_reward"], p["hit_reward"])
        self._dirs = _dirs(self.n_beams, device)
        n = self.n_envs
        self.state = torch.zeros(n, 8, dtype=torch.float64, device=device)
        self.counters = torch.zeros(n, 4, dtype=torch.int64, device=device)
        self.counters[:, 2] = TIMELIMITED                 # nothing runs before the first reset
        self.obs = torch.zeros(n, self.obs_dim, dtype=torch.float32, device=device)
        self.tallies = torch.zeros(n, 4, dtype=torch.float64, device=device)
        self.returns = torch.zeros(n, dtype=torch.float64, device=device)   # the running return of each robot's episode

    def _world_args(self):
        w = self.world
        return (N.ptr(w.segments), w.segments.shape[0], N.ptr(w.circles), w.circles.shape[0], N.ptr(self._dirs), self._cp,
                self._task, self.seed, self.env_offset)

    def reset(self, mask=None):
        """Reset all robots, or those where `mask` (N,) is set: episode += 1, a new start and goal, the running return
        back to 0.  Returns `obs`."""
        m = None
        if mask is not None:
            _need_cuda(mask)
            if mask.shape != (self.n_envs,):
                raise ValueError(f"mask: expected ({self.n_envs},), got {tuple(mask.shape)}")
            m = mask.to(torch.uint8).contiguous()
        N.check(N.lib().porl_nav_dreset(*self._world_args(), N.ptr(m), N.ptr(self.state), N.ptr(self.counters),
                                        N.ptr(self.obs), self.obs.stride(0), N.ptr(self.returns), self.n_envs,
                                        N.current_stream_ptr(self.state)), "porl_nav_dreset")
        return self.obs

    def step(self, actions, replay=None):
        """One step of every running robot with `actions` (N,) int64 on the device; an index outside [0, n_actions) is
        clamped into range.  `replay`: an optional DeviceReplay with rows of obs_dim floats and capacity >= N; robot i's
        transition `[obs acted on, clamped action, reward, obs reached, terminated | truncated]` goes into slot
        (replay.position + i) % capacity and the ring advances by N (a finished robot without auto_reset writes nothing:
        its slot keeps what it held).  Returns NavStep; `sim.obs` is what to act on next."""
        _need_cuda(actions)
        n, S = self.n_envs, self.obs_dim
        if actions.shape != (n,) or actions.dtype != torch.int64:
            raise ValueError(f"actions: expected ({n},) int64, got {actions.dtype} {tuple(actions.shape)}")
        actions = actions.contiguous()
        mirror, base = None, 0
        if replay is not None:
            if replay.states.device != self.state.device or replay.state_dim != S:
                raise ValueError(f"replay: need rows of {S} floats on {self.device}")
            if n > replay.capacity:
                raise ValueError(f"replay: {n} robots > capacity {replay.capacity}: two robots would share a slot")
            mirror, base = C.byref(replay.mirror()), replay.position
        dev = self.device
        next_obs = torch.empty(n, S, dtype=torch.float32, device=dev)
        reward = torch.empty(n, dtype=torch.float32, device=dev)
        flags = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        N.check(N.lib().porl_nav_dstep(*self._world_args(), N.ptr(actions), N.ptr(self.state), N.ptr(self.counters),
                                       N.ptr(self.obs), self.obs.stride(0), N.ptr(next_obs), S, N.ptr(reward), N.ptr(flags),
                                       N.ptr(status), mirror, base, N.ptr(self.tallies), N.ptr(self.returns), n,
                                       N.current_stream_ptr(self.state)), "porl_nav_dstep")
        if replay is not None:
            replay.advance(n)
        return NavStep(next_obs, reward, (flags & 1).bool(), (flags & 2).bool(), status)

    def set_state(self, state=None, counters=None, obs=None, tallies=None, returns=None):
        """Overwrite the resident state / counters / observation / tallies / running returns (tests and restarts)."""
        for dst, src in ((self.state, state), (self.counters, counters), (self.obs, obs), (self.tallies, tallies),
                         (self.returns, returns)):
            if src is not None:
                dst.copy_(torch.as_tensor(src).to(dst.device, dst.dtype).reshape(dst.shape))


class Env:
    """`Env(action_size, state_size, rank_update_interval, namespace)` of env/env.py on one robot of a
    DiscreteLidarNavSim: the gymnasium protocol with numpy and Python scalars, `cur_episode`, and `rank`, which grows by
    one after every `rank_update_interval` resets and moves the robot to `NavWorld.lattice(rank)`'s square (:234-235,
    :288-292).  `state_size` must be n_beams + 2 (362).  gymnasium is not imported."""

    def __init__(agent, action_size, state_size, rank_update_interval=150, namespace="tb3", seed=0, device="cuda", **params):
        agent.action_size, agent.state_size = int(action_size), int(state_size)
        agent.rank_update_interval, agent.namespace = int(rank_update_interval), namespace
        if agent.rank_update_interval < 1:
            raise ValueError("rank_update_interval must be positive")
        agent.status = "initialized"
        agent.map_x, agent.map_y = -10., -10.
        agent.rank, agent.cur_step, agent.cur_episode = 0, 0, 0
        agent._seed, agent._device, agent._params = seed, device, dict(params)
        agent.sim = agent._make_sim()
        if agent.sim.obs_dim != agent.state_size:
            raise ValueError(f"state_size {state_size}: the observation is n_beams + 2 = {agent.sim.obs_dim} floats")
        p = agent.sim.params
        agent.min_range, agent.episode_step = p["min_range"], p["episode_step"]
        agent._action = torch.zeros(1, dtype=torch.int64, device=agent.sim.device)

    def _make_sim(agent):
        world = NavWorld.lattice(rank=agent.rank, map_x=agent.map_x, map_y=agent.map_y)
        agent._sim_rank = agent.rank
        return DiscreteLidarNavSim(world, 1, n_actions=agent.action_size, seed=agent._seed, auto_reset=False,
                                   device=agent._device, **agent._params)

    def _info(agent, status):
        agent.status = STATUS_NAMES[int(status) & 0xff]
        return {"status": agent.status}

    def reset(agent, seed=None, options=None):
        if agent._sim_rank != agent.rank:                             # the square of the new rank, from this reset on
            old = agent.sim
            agent.sim = agent._make_sim()
            agent.sim.set_state(counters=old.counters, tallies=old.tallies)   # the episode number keys the draws: keep counting
        state = agent.sim.reset()[0].cpu().numpy()
        agent.cur_step = 0
        agent.cur_episode += 1
        if agent.cur_episode % agent.rank_update_interval == 0:       # :234-235: the NEXT reset draws in the next square
            agent.rank += 1
        return state, agent._info(0)

    def step(agent, action):
        agent._action.fill_(int(action))
        out = agent.sim.step(agent._action)
        host = torch.cat([out.next_obs[0].double(), out.reward.double(), out.status.double(),
                          out.terminated.double(), out.truncated.double()]).cpu().numpy()   # one copy per step
        S = agent.sim.obs_dim
        agent.cur_step += 1
        return (host[:S].astype(np.float32), float(host[S]), bool(host[S + 2]), bool(host[S + 3]), agent._info(host[S + 1]))

    def render(agent):
        pass

    def close(agent):
        pass
