"""`Env` of the reference's env/gazebo.py as an N = 1 `LidarNavSim`: the constructor's arguments in its order, the
gymnasium protocol (`reset() -> (state, info)`, `step(action) -> (state, reward, terminated, truncated, info)`), numpy in
and out, `info["status"]` one of running | hit | goal | timelimited.  No ROS, no Gazebo, and gymnasium is not imported.

`timelimited` is reported where the reference leaves `running` when the step limit ends an episode.
"""
from __future__ import annotations

import numpy as np
import torch

from .navsim import STATUS_NAMES, LidarNavSim, NavWorld


class Env:
    def __init__(agent, namespace, state_size, action_size, rank=0, world=None, seed=0, device="cuda", **params):
        agent.namespace = namespace
        agent.state_size, agent.action_size, agent.rank = state_size, action_size, rank
        agent.status = "initialized"
        agent.map_x, agent.map_y = -10., -10.
        if world is None:
            world = NavWorld.lattice(rank=rank, map_x=agent.map_x, map_y=agent.map_y)
        # every process of collect.py draws from its own stream: the robot's index in the stream's key is its rank
        agent.sim = LidarNavSim(world, 1, seed=seed, env_offset=rank, layout="goal", auto_reset=False, device=device, **params)
        p = agent.sim.params
        agent.max_lin_vel, agent.max_ang_vel = p["max_lin_vel"], p["max_ang_vel"]
        agent.min_range, agent.episode_step = p["min_range"], p["episode_step"]
        agent.cur_step, agent.cur_episode = 0, 0
        agent._action = torch.zeros(1, 2, dtype=torch.float32, device=agent.sim.device)

    def _info(agent, status):
        agent.status = STATUS_NAMES[int(status) & 0xff]
        return {"status": agent.status}

    def step(agent, action):
        """action (2,): linear velocity [m/s] and angular velocity [rad/s], as the reference publishes them."""
        agent._action.copy_(torch.as_tensor(np.asarray(action, dtype=np.float32).reshape(1, 2)))
        out = agent.sim.step(agent._action)
        host = torch.cat([out.next_obs[0].double(), out.reward.double(), out.status.double(),
                          out.terminated.double(), out.truncated.double()]).cpu().numpy()   # one copy per step
        S = agent.sim.obs_dim
        agent.cur_step += 1
        return (host[:S].astype(np.float32), float(host[S]), bool(host[S + 2]), bool(host[S + 3]), agent._info(host[S + 1]))

    collect_step = step

    def reset(agent, seed=None, options=None):
        state = agent.sim.reset()[0].cpu().numpy()
        agent.cur_step = 0
        agent.cur_episode += 1
        return state, agent._info(0)

    def render(agent):
        pass

    def close(agent):
        pass
