"""Rolling a trained agent out in the task: the reference's test.py (`evaluate_policy`, called every few epochs by
por_train.py:96-98 and sorl_train.py:73-75) on the device simulator of porl_amd/env, and a batched form that runs N robots
per round with one device-to-host copy per round.
"""
from __future__ import annotations

import statistics

import numpy as np
import torch

from .env.gazebo import Env
from .env.navsim import GOAL


def _check_limit(episode_step, sim_limit):
    if episode_step > sim_limit:
        raise ValueError(f"episode_step {episode_step} exceeds the simulator's own step limit {sim_limit}: a robot it stops "
                         "idles with reward 0, where the reference's environment goes on stepping; raise the simulator's")


def evaluate_policy(agent, args, env=None):
    """What the reference's test.py:8-53 measures, in its order of operations: `args.test_episodes` roll-outs of at most
    `args.episode_step` steps; each step asks `agent.select_action` for an action in [-1, 1]^2 and maps it to the command
    `v = (a0 + 1) * max_lin_vel / 2`, `w = a1 * max_ang_vel`, which must lie inside the robot's limits (AssertionError
    otherwise, as upstream); a roll-out ends when the environment terminates or at the last permitted step.  Returns
    (mean index of the final step, mean summed reward, fraction that ended with status `goal`).  `env`: the `Env` to roll
    out in (default: a new one in the lattice world with the reference's constructor arguments)."""
    if env is None:
        env = Env(args.namespace, args.state_size, args.action_size, device=getattr(args, "device", "cuda"))
    _check_limit(args.episode_step, env.episode_step)
    half_v, max_w = env.max_lin_vel / 2, env.max_ang_vel
    last_step = args.episode_step - 1
    outcomes = []                                          # one (final step, return, reached the goal) per roll-out
    for _ in range(args.test_episodes):
        obs, _ = env.reset()
        ret = 0
        for t in range(args.episode_step):
            on_device = torch.from_numpy(obs).to(device=args.device, dtype=torch.float32)
            a = agent.select_action(on_device.unsqueeze(0))[0]
            v, w = (float(a[0]) + 1.0) * half_v, float(a[1]) * max_w
            if not 0 <= v <= env.max_lin_vel:
                raise AssertionError(f"policy commands v = {v} m/s, outside [0, {env.max_lin_vel}]")
            if not -max_w <= w <= max_w:
                raise AssertionError(f"policy commands w = {w} rad/s, outside [-{max_w}, {max_w}]")
            obs, reward, terminated, _, info = env.step(np.array([v, w]))
            ret += reward
            if terminated or t == last_step:
                outcomes.append((t, ret, float(info["status"] == "goal")))
                break
    return tuple(statistics.fmean(o[k] for o in outcomes) for k in range(3))


def evaluate_policy_batched(act, sim, episodes, episode_step):
    """The same triple from `episodes` episodes run N = sim.n_envs at a time (the last round uses the first robots only).
    `act`: obs (N, S) -> commands (N, 2) `v, w` on the device, already in the robot's units.  `sim` runs without
    auto_reset: a finished robot idles until the round ends.  `episode_step` may not exceed the simulator's own step limit
    (ValueError): a robot that limit stops would idle where the reference's goes on.  Per round everything stays on the
    device; one copy brings the round's steps, scores and outcomes to the host."""
    if sim.auto_reset:
        raise ValueError("evaluate_policy_batched needs a simulator with auto_reset=False")
    if episodes < 1 or episode_step < 1:
        raise ValueError("episodes and episode_step must be positive")
    _check_limit(episode_step, sim.params["episode_step"])
    n, dev = sim.n_envs, sim.device
    scores, success, steps = [], [], []
    left = episodes
    while left > 0:
        take = min(n, left)
        sim.reset()
        score = torch.zeros(n, dtype=torch.float64, device=dev)
        last = torch.full((n,), episode_step - 1, dtype=torch.int64, device=dev)      # unless it terminates earlier
        for t in range(episode_step):
            out = sim.step(act(sim.obs).to(torch.float32))
            score += out.reward.double()                  # a finished robot idles: its later rewards are 0
            last = torch.where(out.terminated, torch.full_like(last, t), last)       # fires once: the robot idles after
        goal = (sim.counters[:, 2] & 0xff) == GOAL
        host = torch.stack([last.double(), score, goal.double()])[:, :take].cpu().numpy()
        steps += host[0].tolist()
        scores += host[1].tolist()
        success += host[2].tolist()
        left -= take
    return statistics.fmean(steps), statistics.fmean(scores), statistics.fmean(success)


def evaluate_discrete(trainer, sim, episodes, episode_step=None, seed=0, constrained=True, poll_every=0):
    """Score a trained agent of the discrete task (env/env.py) by its GREEDY policy: `episodes` episodes of at most
    `episode_step` steps (default: the simulator's own limit) run in rounds of N = sim.n_envs, one episode per robot; the
    last round counts the first robots only.  `sim`: a DiscreteLidarNavSim with auto_reset=False whose observation and
    action count are the trainer's; `episode_step` may not exceed its step limit (ValueError).

    Per round: sim.reset(), sim.tallies zeroed, then `episode_step` iterations of the act call the trainer's own vectorised
    loop makes (train.vector_offline.batched_act) at epsilon 0, and sim.step.  For a BCQTrainer `constrained=True` scores the
    policy its learn step's target assumes, False the plain arg-max the reference's trainer acts with.  `seed` keys the
    fractions of an IQN agent (with sim.env_offset + i and the act-step, counted through the rounds).  A finished robot is
    frozen by the step kernel, so when the round ends counters[:, 0] is every episode's length, the tallies hold return, goal
    and hit of a finished episode and sim.returns the return of one still running: nothing is computed in torch inside the
    loop, and one copy per round brings the results to the host.  `poll_every` = k > 0 adds one read-back of "every robot has
    finished" after every k-th iteration and ends the round there; the results are the same.  The trainer's parameters,
    epsilon, counters and replay are not touched.

    Returns a dict: the means `steps` (episode length), `score` (summed reward), `success` (reached the goal), `hits`
    (collided), `timeouts` (neither), and the per-episode numpy arrays `episode_steps`, `episode_scores`, `episode_goals`,
    `episode_hits`."""
    from .train.vector_offline import batched_act
    if sim.auto_reset:
        raise ValueError("evaluate_discrete needs a simulator with auto_reset=False")
    if episode_step is None:
        episode_step = int(sim.params["episode_step"])
    if episodes < 1 or episode_step < 1 or poll_every < 0:
        raise ValueError("episodes and episode_step must be positive, poll_every not negative")
    _check_limit(episode_step, sim.params["episode_step"])
    n, dev = sim.n_envs, sim.device
    eng, A, act = batched_act(trainer, n, constrained=constrained)
    if sim.obs_dim != eng.cfg.state_dim or sim.n_actions != A:
        raise ValueError(f"the simulator observes {sim.obs_dim} floats and takes {sim.n_actions} actions; the trainer's network "
                         f"maps {eng.cfg.state_dim} to {A}")
    if sim.state.device != eng.device:
        raise ValueError(f"simulator on {sim.state.device}, trainer on {eng.device}")
    actions = torch.empty(n, dtype=torch.int64, device=dev)
    rows, t0, left = [], 0, episodes
    while left > 0:
        take = min(n, left)
        sim.reset()
        sim.tallies.zero_()
        for k in range(episode_step):
            act(sim.obs, 0.0, seed, t0 + k, sim.env_offset, actions)
            sim.step(actions)
            if poll_every and (k + 1) % poll_every == 0 and bool(((sim.counters[:, 2] & 0xff) != 0).all()):
                break
        # a finished episode's return sits in its tallies row and its running return is 0; one still running the other way
        host = torch.cat([sim.counters[:, :1].double(), sim.tallies[:, 1:2] + sim.returns[:, None], sim.tallies[:, 2:4]],
                         dim=1)[:take].cpu().numpy()
        rows.append(host)
        left -= take
        t0 += episode_step                                 # act-step numbers do not depend on where a poll ended a round
    host = np.concatenate(rows, axis=0)
    steps, scores, goals, hits = host[:, 0].astype(np.int64), host[:, 1].copy(), host[:, 2] != 0, host[:, 3] != 0
    return dict(steps=statistics.fmean(steps.tolist()), score=statistics.fmean(scores.tolist()),
                success=statistics.fmean(goals.tolist()), hits=statistics.fmean(hits.tolist()),
                timeouts=statistics.fmean((~goals & ~hits).tolist()),
                episode_steps=steps, episode_scores=scores, episode_goals=goals, episode_hits=hits)


_command_consts: dict = {}


def _to_command(mean):
    """`v = (a0 + 1) * 0.075`, `w = a1 * 1.5` on device tensors; the two constants are uploaded once per device."""
    key = (mean.device, mean.dtype)
    if key not in _command_consts:
        _command_consts[key] = (torch.tensor([1., 0.], device=mean.device, dtype=mean.dtype),
                                torch.tensor([0.15 / 2, 1.5], device=mean.device, dtype=mean.dtype))
    shift, scale = _command_consts[key]
    return (mean + shift) * scale


def sorl_act(agent):
    """obs -> command for a SORL agent: the policy mean through `policy.act(..., deterministic=True)`, on the device."""
    def act(obs):
        agent.flush()
        x = agent.backbone(obs) if getattr(agent, "backbone", None) is not None else obs
        return _to_command(agent.policy.act(x, deterministic=True))
    return act


def por_act(agent):
    """obs -> command for a POR agent with its action policy set (`POR.set_execute_policy`): the action policy's mean on
    `[obs | goal_policy mean(obs)]`, as `select_action` forms it, on the device."""
    def act(obs):
        bc = agent.__dict__.get("_execute_policy")
        if bc is None:
            raise RuntimeError("por_act: no action policy is set (POR.set_execute_policy)")
        agent.flush()
        bc.flush()
        goal = agent.goal_policy.act(obs, deterministic=True)
        return _to_command(bc.policy.act(torch.cat([obs, goal], dim=-1), deterministic=True))
    return act
