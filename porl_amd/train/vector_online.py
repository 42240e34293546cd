"""`train_vectorized`: the Q-learning trainers in the discrete lidar task (env/env.py) with N robots per step and no host
synchronisation inside the loop.

One iteration is three native calls on the current stream:
  act      QnetEngine.act_rows on `sim.obs` — the batched forward and the epsilon-greedy rule (porl_qnet_act_rows); the
           actions stay on the device;
  step     DiscreteLidarNavSim.step(actions, replay=...) — one launch moves every robot, scans, rewards, resets the robots
           that finished and writes each transition straight into the replay arrays (porl_nav_dstep);
  learn    `learn_per_step` steps once len(replay) >= learning_starts: the step kernel draws its minibatch from the replay
           arrays itself (QnetEngine.learn_sampled with the trainer's `_rows_variant()`, so Double DQN stays Double) when
           the engine can sample; a network on the one-launch kernel that cannot takes engine.sample_indices and
           learn_indexed; a network off the one-launch kernel takes sample_indices, a gather and the trainer's `learn_on` —
           the choices CQLTrainer.learn_device_sampled makes.
Each learn step's mean loss is copied device-to-device into a loss log.  Nothing is read back before the end.

The reference's loop (dqn_trainer.py:119-180) decays epsilon and synchronises the target network once per EPISODE.  N robots
end their episodes at different steps, so that schedule has no meaning here and a BLOCK of `block` iterations takes the
episode's place: after every block, on the host and without waiting, epsilon = max(epsilon_min, epsilon * epsilon_decay),
and the target network is synchronised after block b when b % update_target_freq == 0 (b counts from 0, as the reference's
episode number does).

Plain-Q trainers only: CQLTrainer, DQNTrainer, DDQNTrainer, DDDQNTrainer.  PERTrainer has the same loop around its own
memory as `train_vectorized_per` (train/vector_per.py), C51Trainer and QRDQNTrainer around their own act and learn calls as
`train_vectorized_dist` (train/vector_dist.py), IQNTrainer on its own engine as `train_vectorized_iqn`
(train/vector_iqn.py); all three share `check_sim`, `check_starts` and `end_of_step` below.  BCQ is offline: train/vector_offline.py.
"""
from __future__ import annotations

import torch

from .. import engine as E
from ..buffer.device_replay import DeviceReplay


def _refuse(trainer):
    from .bcq_trainer import BCQTrainer
    from .cql_trainer import CQLTrainer
    from .dqn_per_trainer import PERTrainer
    if not isinstance(trainer, CQLTrainer) or isinstance(trainer, (PERTrainer, BCQTrainer)):
        raise NotImplementedError(
            f"train_vectorized covers the plain-Q trainers (CQL, DQN, Double DQN, Dueling); {type(trainer).__name__} runs in "
            "this task through train_online(Env(...)) (porl_amd.env.Env, the single-robot form of the same simulator)")
    if trainer._exchange.active:
        raise NotImplementedError("train_vectorized has no gradient exchange; use train_online(Env(...)) per rank")


def _gather(replay, idx):
    """The minibatch `idx` of a DeviceReplay as five tensors (ReplayBuffer.gather_device's kernels)."""
    B = idx.numel()
    return (E.gather_rows(replay.states, idx), E.gather_rows(replay.actions.view(torch.float32).view(-1, 2), idx).view(torch.int64).view(B),
            E.gather_rows(replay.rewards.view(-1, 1), idx).view(B), E.gather_rows(replay.next_states, idx),
            E.gather_rows(replay.dones.view(-1, 1), idx).view(B))


def learn_step(trainer, replay, seed, draw):
    """One learn step of `trainer` on batch_size distinct rows of the first len(replay) rows of `replay`, drawn by the
    keyed permutation (seed, draw); no read-back.  The mean loss is left in trainer._engine.stats[0]."""
    eng, B = trainer._engine, trainer.batch_size
    if not eng.fused:
        idx = E.sample_indices(len(replay), B, seed, draw, device=eng.device)
        held, trainer.async_losses = trainer.async_losses, True       # learn_on returns the device statistics, unread
        try:
            trainer.learn_on(*_gather(replay, idx))
        finally:
            trainer.async_losses = held
        return
    hp = trainer.optimizer.hyper(trainer.gamma, float(trainer.alpha), 1.0 / B)
    if eng.can_sample:
        eng.learn_sampled(hp, *replay.arrays(), len(replay), B, seed, draw, variant=trainer._rows_variant())
    else:
        idx = E.sample_indices(len(replay), B, seed, draw, device=eng.device)
        eng.learn_indexed(hp, *replay.arrays(), idx, variant=trainer._rows_variant())
    trainer.optimizer.step_count = hp.step


def check_sim(eng, sim, n_steps, block, learn_per_step, who, n_actions=None):
    """The argument checks the vectorised loops share (`who` names the loop in the one message that names it).  `n_actions`:
    the trainer's action count where it is not the network's output count (a distributional head)."""
    S = sim.obs_dim
    n_actions = eng.cfg.n_actions if n_actions is None else n_actions
    if not sim.auto_reset:
        raise ValueError(f"{who} needs a simulator with auto_reset=True")
    if S != eng.cfg.state_dim or sim.n_actions != n_actions:
        raise ValueError(f"the simulator observes {S} floats and takes {sim.n_actions} actions; the trainer's network maps "
                         f"{eng.cfg.state_dim} to {n_actions}")
    if sim.state.device != eng.device:
        raise ValueError(f"simulator on {sim.state.device}, trainer on {eng.device}")
    if n_steps < 1 or block < 1 or learn_per_step < 0:
        raise ValueError("n_steps and block must be positive, learn_per_step not negative")


def check_starts(trainer, learning_starts, capacity):
    """The first buffer size at which a learn step runs: never below batch_size, never above `capacity`."""
    starts = max(trainer.batch_size, int(trainer.training_learning_step if learning_starts is None else learning_starts))
    if starts > capacity:
        raise ValueError(f"learning_starts {starts} > replay capacity {capacity}: no learn step would ever run")
    return starts


def end_of_step(trainer, t, block):
    """Close act-step t: advance the counter and, when a block ends, apply the reference's per-episode schedule."""
    trainer._vec_steps = t + 1
    if trainer._vec_steps % block == 0:
        b = trainer._vec_steps // block - 1
        trainer.epsilon = max(trainer.epsilon_min, trainer.epsilon * trainer.epsilon_decay)
        if b % trainer.update_target_freq == 0:
            trainer.sync_target()


def train_vectorized(trainer, sim, n_steps, replay=None, learn_per_step=1, learning_starts=None, block=32, seed=0):
    """Run `n_steps` iterations of act -> step -> learn (module docstring) with `sim`, a DiscreteLidarNavSim with
    auto_reset=True whose observation and action count are the trainer's.  `replay`: a DeviceReplay (default: one of the
    trainer's replay capacity, kept as `trainer.device_replay`); `learning_starts` defaults to the trainer's
    training_learning_step, and is never below batch_size.  `seed` keys the exploration draws (with sim.env_offset + i
    and the act-step) and the minibatch draws.  Act-step, draw and block counters live on the trainer, so a second call
    continues the first.  Returns, after the one read-back, a dict: losses (numpy, one mean loss per learn step), tallies
    (numpy (4,): sim.tallies summed over robots — episodes, sum of returns, goals, hits), transitions, learn_steps."""
    _refuse(trainer)
    eng = trainer._engine
    N_, S = sim.n_envs, sim.obs_dim
    check_sim(eng, sim, n_steps, block, learn_per_step, "train_vectorized")
    if replay is None:
        replay = getattr(trainer, "device_replay", None)
        if replay is None:
            replay = DeviceReplay(max(int(getattr(trainer.replay_buffer, "capacity", 100000)), N_), S, eng.device)
    starts = check_starts(trainer, learning_starts, replay.capacity)
    trainer.device_replay = replay
    eng._ensure_bound()
    if bool((sim.counters[:, 2] & 0xff != 0).any()):                 # before the loop: robots that are not running
        sim.reset()
    dev = eng.device
    q = torch.empty(N_, eng.cfg.n_actions, dtype=torch.float32, device=dev)
    actions = torch.empty(N_, dtype=torch.int64, device=dev)
    loss_log = torch.zeros(max(1, n_steps * learn_per_step), dtype=torch.float32, device=dev)
    n_learn = 0
    for _ in range(n_steps):
        t = trainer._vec_steps = getattr(trainer, "_vec_steps", 0)
        eng.act_rows(sim.obs, trainer.epsilon, seed, t, env_offset=sim.env_offset, q=q, out=actions)
        sim.step(actions, replay=replay)
        if len(replay) >= starts:
            for _k in range(learn_per_step):
                trainer._draws = getattr(trainer, "_draws", 0)
                learn_step(trainer, replay, seed, trainer._draws)
                trainer._draws += 1
                loss_log[n_learn:n_learn + 1].copy_(eng.stats[:1])
                n_learn += 1
        end_of_step(trainer, t, block)                                # a block ends: the reference's per-episode schedule
    host = torch.cat([loss_log[:n_learn].double(), sim.tallies.sum(0)]).cpu().numpy()      # the one read-back
    return dict(losses=host[:n_learn].astype("float32"), tallies=host[n_learn:], transitions=N_ * n_steps, learn_steps=n_learn)
