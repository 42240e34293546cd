"""The offline half in the discrete lidar task (env/env.py), on the device: collect a data set with N robots, learn from it
without stepping, and hand every trainer family one batched act call (evaluate.evaluate_discrete scores agents with it).

  collect_discrete      `n_steps` iterations of act -> DiscreteLidarNavSim.step(actions, replay=...): every transition goes
                        straight into a DeviceReplay.  Without a trainer every action is the exploration draw of
                        porl_qnet_select — the device form of collect_dataset's random policy (reference policy/bcq.py:8-20);
                        with a trainer of any family that family's batched act call at `epsilon`, which is how a behaviour
                        data set of mixed quality is made; with `expert`, an env.expert.AStarExpert of the simulator, the
                        expert's score table under the same epsilon-greedy rule: goal-reaching data without a trained agent.
  train_offline_device  the reference's offline pipeline after the collection (scripts/train_bcq.py: bcq_behavior_pretrain,
                        then bcq_learn in DQNTrainer.train_offline's loop) on a DeviceReplay: the choices of
                        bcq_pretrain_device_sampled and bcq_learn_device_sampled (policy/bcq.py) with the replay arrays in place
                        of a ReplayBuffer mirror; for the plain-Q trainers (CQL, DQN, Double DQN, Dueling) `learn_step` of
                        train/vector_online.py.  The target network is synchronised when i % update_target_freq == 0, as
                        online.run_offline does; each loss is copied device to device into a log that is read back once.

Minibatches are the keyed permutation's (engine.sample_indices): `seed` and the draw counter `trainer._draws`, which the
other device-sampled entry points share, so a second call continues the first.  Nothing is read back inside a loop.
"""
from __future__ import annotations

import math

import torch

from .. import _native as N
from .. import engine as E
from ..buffer.device_replay import DeviceReplay
from .vector_online import check_sim, draw_count, family_of, learn_step


def batched_act(trainer, n_envs, constrained=True):
    """(engine, n_actions, act) for `trainer`: act(obs, epsilon, seed, t, env_offset, out) is the batched act call the
    trainer's family makes in the vectorised loop for `n_envs` robots (the family table of train/vector_online.py), with its
    scratch tables allocated once, here.  `constrained` is BCQTrainer.act_rows's."""
    fam = family_of(type(trainer))
    if fam is None:
        raise NotImplementedError(f"{type(trainer).__name__} has no batched act call in the discrete task")
    eng = fam.engine(trainer, n_envs)
    if hasattr(eng, "_ensure_bound"):
        eng._ensure_bound()
    return eng, trainer.action_size, fam.act(trainer, eng, n_envs, constrained)


def collect_discrete(sim, replay, n_steps, trainer=None, epsilon=1.0, seed=0, t0=0, expert=None):
    """Run `n_steps` iterations of act -> sim.step(actions, replay=replay) with `sim`, a DiscreteLidarNavSim with
    auto_reset=True, and `replay`, a DeviceReplay of its observation width and at least its robot count.  `trainer=None`:
    uniform random actions (engine.qnet_select with epsilon 1 on a dummy value table, no forward); else the trainer's batched
    act call (`batched_act`) at `epsilon` — the trainer is read, never modified.  `expert` (without a trainer; both: ValueError):
    an AStarExpert of `sim`; the act is `expert()` into a scratch table, then engine.qnet_select on it at `epsilon` — the nearest
    turn to the planned waypoint, or with probability epsilon the same uniform draw (epsilon 1: the random policy, action for
    action).  Act-step k of this call is `t0 + k`: with
    `seed` and sim.env_offset + i it keys robot i's exploration draws, so a later call continues with t0 advanced by n_steps.
    Returns, after the one read-back, dict(transitions, tallies) — tallies (numpy (4,)): sim.tallies summed over robots."""
    if n_steps < 1 or t0 < 0:
        raise ValueError("n_steps must be positive, t0 not negative")
    if not 0.0 <= epsilon <= 1.0:
        raise ValueError("epsilon must lie in [0, 1]")
    if expert is not None and trainer is not None:
        raise ValueError("collect_discrete: pass a trainer or an expert, not both")
    N_, dev = sim.n_envs, sim.device
    if expert is not None:
        if not sim.auto_reset:
            raise ValueError("collect_discrete needs a simulator with auto_reset=True")
        if expert.sim is not sim or not expert.discrete:
            raise ValueError("collect_discrete: the expert must have been made for this DiscreteLidarNavSim")
        table = torch.empty(N_, sim.n_actions, dtype=torch.float32, device=dev)
        act = lambda obs, eps, seed_, t, env_offset, out: E.qnet_select(expert(out=table), eps, seed_, t, env_offset=env_offset,
                                                                         out=out)
    elif trainer is None:
        if not sim.auto_reset:
            raise ValueError("collect_discrete needs a simulator with auto_reset=True")
        dummy = torch.zeros(N_, sim.n_actions, dtype=torch.float32, device=dev)
        act = lambda obs, eps, seed_, t, env_offset, out: E.qnet_select(dummy, 1.0, seed_, t, env_offset=env_offset, out=out)
    else:
        eng, A, act = batched_act(trainer, N_)
        check_sim(eng, sim, n_steps, 1, 0, "collect_discrete", n_actions=A)
    if bool((sim.counters[:, 2] & 0xff != 0).any()):                 # before the loop: robots that are not running
        sim.reset()
    actions = torch.empty(N_, dtype=torch.int64, device=dev)
    for k in range(n_steps):
        act(sim.obs, epsilon, seed, t0 + k, sim.env_offset, actions)
        sim.step(actions, replay=replay)
    return dict(transitions=N_ * n_steps, tallies=sim.tallies.sum(0).cpu().numpy())      # the one read-back


def _refuse(trainer):
    from .cql_trainer import CQLTrainer
    from .dist_trainer import DistTrainerBase
    from .dqn_per_trainer import PERTrainer
    from .iqn_trainer import IQNTrainer
    name = type(trainer).__name__
    if isinstance(trainer, PERTrainer):
        raise NotImplementedError(f"train_offline_device draws uniform minibatches; {name} learns from its own prioritized "
                                  "memory in train_vectorized_per")
    if isinstance(trainer, DistTrainerBase):
        raise NotImplementedError(f"train_offline_device covers BCQ and the plain-Q trainers; {name} learns in train_vectorized_dist")
    if isinstance(trainer, IQNTrainer):
        raise NotImplementedError(f"train_offline_device covers BCQ and the plain-Q trainers; {name} learns in train_vectorized_iqn")
    if not isinstance(trainer, CQLTrainer):
        raise NotImplementedError(f"train_offline_device covers BCQ and the plain-Q trainers (CQL, DQN, Double DQN, Dueling), "
                                  f"not {name}")
    if trainer._exchange.active:
        raise NotImplementedError("train_offline_device has no gradient exchange; use train_offline per rank")


def _next_draw(trainer):
    draw = draw_count(trainer)
    trainer._draws = draw + 1
    return draw


def train_offline_device(trainer, replay, n_iters, seed=0, pretrain=None):
    """`n_iters` learn steps of `trainer` on the first len(replay) rows of `replay`, a DeviceReplay (module docstring).  A
    BCQTrainer first takes `pretrain` cross-entropy steps of its behaviour policy (default: trainer.num_epochs), then BCQ steps
    with the mask at trainer.threshold; a plain-Q trainer takes `learn_step`.  PER, C51, QR-DQN and IQN trainers and an active
    gradient exchange raise NotImplementedError.  Returns, after the one read-back, dict(losses, pretrain_losses, learn_steps):
    losses (numpy float32, one mean loss per learn step), pretrain_losses (numpy float64, the cross-entropy per pre-training
    step as bcq_pretrain_device_sampled reports it: the fp32 statistic + ln A; empty for a plain-Q trainer)."""
    from .bcq_trainer import BCQTrainer
    _refuse(trainer)
    eng, B = trainer._engine, trainer.batch_size
    bcq = isinstance(trainer, BCQTrainer)
    n_pre = (int(trainer.num_epochs) if pretrain is None else int(pretrain)) if bcq else 0
    if n_iters < 0 or n_pre < 0:
        raise ValueError("n_iters and pretrain must not be negative")
    if not isinstance(replay, DeviceReplay) or replay.state_dim != eng.cfg.state_dim or replay.states.device != eng.device:
        raise ValueError(f"replay: need a DeviceReplay with rows of {eng.cfg.state_dim} floats on {eng.device}")
    if B > len(replay):
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    eng._ensure_bound()
    dev, rows = eng.device, len(replay)
    pre_log = torch.zeros(max(n_pre, 1), dtype=torch.float32, device=dev)
    loss_log = torch.zeros(max(n_iters, 1), dtype=torch.float32, device=dev)
    if bcq:
        beh, opt = trainer._behavior_engine, trainer.behavior_optimizer
        beh._ensure_bound()
        var = N.QnetVariant(0, None, None, None, None, 1)              # td_off: loss = penalty = CE - ln A
        for k in range(n_pre):
            draw = _next_draw(trainer)
            hp = opt.hyper(trainer.gamma, 1.0, 1.0 / B)
            if beh.can_sample:
                beh.learn_sampled(hp, *replay.arrays(), rows, B, seed, draw, variant=var)
            else:
                idx = E.sample_indices(rows, B, seed, draw, device=dev)
                beh.learn_indexed(hp, *replay.arrays(), idx, variant=var)
            opt.step_count = hp.step
            pre_log[k:k + 1].copy_(beh.stats[2:3])
    for i in range(n_iters):
        draw = _next_draw(trainer)
        if bcq:
            hp = trainer.optimizer.hyper(trainer.gamma, 0.0, 1.0 / B)
            if eng.can_sample:
                eng.bcq_learn_sampled(beh, hp, *replay.arrays(), rows, B, seed, draw, trainer.threshold)
            else:
                idx = E.sample_indices(rows, B, seed, draw, device=dev)
                eng.bcq_learn_indexed(beh, hp, *replay.arrays(), idx, trainer.threshold)
            trainer.optimizer.step_count = hp.step
        else:
            learn_step(trainer, replay, seed, draw)
        loss_log[i:i + 1].copy_(eng.stats[:1])
        if i % trainer.update_target_freq == 0:
            trainer.sync_target()
    host = torch.cat([pre_log[:n_pre], loss_log[:n_iters]]).cpu().numpy()      # the one read-back
    ln_a = math.log(trainer.action_size)
    return dict(losses=host[n_pre:], pretrain_losses=host[:n_pre].astype("float64") + ln_a, learn_steps=n_iters)
