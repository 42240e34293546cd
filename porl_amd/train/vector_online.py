"""The trainers in the discrete lidar task (env/env.py) with N robots per step and no host synchronisation inside the loop:
one loop (`_run`) and one table of what differs between the trainer families (`FAMILIES`).

One iteration, all on the current stream:
  act      the family's batched act call on `sim.obs`: a forward and the epsilon-greedy rule; the actions stay on the device;
  step     DiscreteLidarNavSim.step(actions, replay=...) — one launch moves every robot, scans, rewards, resets the robots
           that finished and writes each transition straight into the replay arrays (porl_nav_dstep);
  learn    `learn_per_step` of the family's learn steps once len(replay) >= learning_starts, each followed by a
           device-to-device copy of its mean loss (engine.stats[0]) into a loss log.
Nothing is read back before the end.  The counters `_vec_steps` (act-steps) and `_draws` (minibatch draws, shared with the
other device-sampled entry points) live on the trainer, so a second call continues the first.

The reference's loop (dqn_trainer.py:119-180) decays epsilon and synchronises the target network once per EPISODE.  N robots
end their episodes at different steps, so that schedule has no meaning here and a BLOCK of `block` iterations takes the
episode's place: after every block, on the host and without waiting, epsilon = max(epsilon_min, epsilon * epsilon_decay),
and the target network is synchronised after block b when b % update_target_freq == 0 (b counts from 0, as the reference's
episode number does).

The families, by entry point:
  train_vectorized       CQL, DQN, Double DQN, Dueling.  act: QnetEngine.act_rows (porl_qnet_act_rows).  learn: `learn_step` —
                         the step kernel draws its minibatch from the replay arrays itself (learn_sampled with the trainer's
                         `_rows_variant()`, so Double DQN stays Double) when the engine can sample; a network on the
                         one-launch kernel that cannot takes engine.sample_indices and learn_indexed; a network off it takes
                         sample_indices, a gather and the trainer's `learn_on` — CQLTrainer.learn_device_sampled's choices.
  train_vectorized_per   PERTrainer, into `trainer.memory`.  act: as above.  step adds one launch that gives the N new leaves
                         the priority of a new row and recomputes their ancestors (PrioritizedReplayBuffer.advance ->
                         porl_per_fill_range).  learn: memory.sample_slots_keyed (tree walk, weights and their mean, the
                         uniforms drawn in the kernel), the weighted Double-DQN step learn_indexed on the store's rows with
                         PERTrainer.learn's choice between per_sample_weights and the reference's broadcast (mean weight),
                         |TD| out, and memory.update_priorities_device.  On a network the one-launch step kernel takes that
                         is 6 launches per iteration with one learn step (forward + select, step, fill, sample, learn,
                         write-back) and the loss copy; a wider network adds its layers' launches to act and learn.
  train_vectorized_dist  C51Trainer, QRDQNTrainer.  act: QnetEngine.act_rows_dist with `_dist_head()` — one wave per robot
                         turns its A x n_sub quantiles / atom logits into A values (csrc/dist_act.hpp), in the order the loss
                         heads rank the next state's actions by, so acting and bootstrapping agree.  learn:
                         dist_learn_sampled, the trainer's learn_on from one native call whose gather launch draws the
                         minibatch.  `learning_starts=None` is the threshold of the trainer's own train_online: batch_size
                         for C51 (c51_trainer.py:205), training_learning_step for QR-DQN (dqn_trainer.py:148).
  train_vectorized_iqn   IQNTrainer, on an IqnEngine of max_batch max(batch_size, min(N, MAX_CHUNK)).  act: IqnEngine.act_rows
                         with num_quantiles_n_policy fractions per robot, per chunk of max_batch robots one staging launch,
                         the layers and one wave per robot for the K x A quantile values.  learn: IqnEngine.learn_sampled.
                         The fractions tau, tau', tau'' are not torch.rand's: robot `sim.env_offset + i` at act-step t and
                         minibatch row b of learn-draw d own fixed elements of the stream keyed by `seed`
                         (csrc/iqn_vector.hpp), so a run does not depend on torch's generator, on chunking, or on how robots
                         are split over simulators.
  (none)                 BCQTrainer is offline: it has an act call, BCQTrainer.act_rows(constrained=...), and no learn step
                         here (train/vector_offline.py).
`batched_act` (train/vector_offline.py) hands out the same act call, so collecting and scoring act as the loop does.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import partial
from typing import Callable, Optional

import torch

from .. import _native as N
from .. import engine as E
from ..buffer.device_replay import DeviceReplay
from ..net.iqn_network import IQNNetwork
from .bcq_trainer import BCQTrainer
from .cql_trainer import CQLTrainer
from .dist_trainer import DistTrainerBase
from .dqn_per_trainer import PERTrainer
from .iqn_trainer import IQNTrainer

MAX_CHUNK = 1024          # robots per IQN forward chunk: the engine's max_batch is max(batch_size, min(n_envs, MAX_CHUNK))


# ---- what the loops share ------------------------------------------------------------------------------------------------
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


def draw_count(trainer):
    """The number of the trainer's next minibatch draw: the counter the device-sampled entry points share, made on first use.
    The caller advances `trainer._draws` once the draw is spent."""
    trainer._draws = getattr(trainer, "_draws", 0)
    return trainer._draws


def _no_exchange(trainer, loop):
    if trainer._exchange.active:
        raise NotImplementedError(f"{loop} has no gradient exchange; use train_online(Env(...)) per rank")


def _new_replay(trainer, sim, eng, replay):
    """`replay`, else the trainer's `device_replay`, else a DeviceReplay of the trainer's replay capacity."""
    if replay is None:
        replay = getattr(trainer, "device_replay", None)
        if replay is None:
            replay = DeviceReplay(max(int(getattr(trainer.replay_buffer, "capacity", 100000)), sim.n_envs), sim.obs_dim, eng.device)
    return replay


def _keep_replay(trainer, replay):
    trainer.device_replay = replay


def _qnet_engine(trainer, n_envs):
    return trainer._engine


# ---- plain Q: CQL, DQN, Double DQN, Dueling ------------------------------------------------------------------------------
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


def _plain_act(trainer, eng, n_envs, constrained=True):
    q = torch.empty(n_envs, trainer.action_size, dtype=torch.float32, device=eng.device)
    return lambda obs, epsilon, seed, t, env_offset, out: eng.act_rows(obs, epsilon, seed, t, env_offset=env_offset, q=q, out=out)


def _plain_learn(trainer, eng):
    return partial(learn_step, trainer)


# ---- PER: the replay is the trainer's sum tree ---------------------------------------------------------------------------
def _per_memory(trainer, sim, eng, replay):
    mem = trainer.memory
    if mem.tree.device != eng.device or mem.state_dim != sim.obs_dim:
        raise ValueError(f"memory: need rows of {sim.obs_dim} floats on {eng.device}")
    if sim.n_envs > mem.capacity:
        raise ValueError(f"{sim.n_envs} robots > memory capacity {mem.capacity}: two robots would share a slot")
    return mem


def _per_prepare(trainer, mem):
    if trainer.batch_size > trainer._td_abs.numel():
        raise ValueError(f"batch_size {trainer.batch_size} > the trainer's |TD| buffer of {trainer._td_abs.numel()}")
    mem.priority_for_new = trainer.max_initial_priority


def _per_learn(trainer, eng):
    B, o = trainer.batch_size, trainer.optimizer
    td_abs, rows = trainer._td_abs[:B], trainer.memory.arrays()

    def learn(mem, seed, draw):
        slots, is_w, wmean, tree_idx = mem.sample_slots_keyed(B, seed, draw)
        hp = o.hyper(trainer.gamma, 0.0, 1.0 / B)
        if trainer.per_sample_weights:
            var = N.QnetVariant(1, is_w.data_ptr(), None, td_abs.data_ptr())
        else:                                                         # the reference's (B,1)*(B,) broadcast: mean(w)*mean(td^2)
            var = N.QnetVariant(1, None, wmean.data_ptr(), td_abs.data_ptr())
        eng.learn_indexed(hp, *rows, slots, variant=var)
        o.step_count = hp.step
        mem.update_priorities_device(tree_idx, td_abs)
    return learn


# ---- C51, QR-DQN: a distributional head on the Q-network engine ----------------------------------------------------------
def _dist_guard(trainer, loop):
    _no_exchange(trainer, loop)
    cls = type(trainer)
    # train_online's guard: the native calls restate the class's own select_action / learn_on
    if cls.learn is not DistTrainerBase.learn or cls._rows_for is None or cls._rows_for is not cls.learn_on or \
            cls._act_for is None or cls._act_for is not cls.select_action:
        raise NotImplementedError(f"{cls.__name__} overrides learn, learn_on or select_action, which {loop}'s "
                                  "native calls do not run; use train_online(Env(...))")


def _dist_act(trainer, eng, n_envs, constrained=True):
    head = trainer._dist_head()
    q = torch.empty(n_envs, trainer.action_size, dtype=torch.float32, device=eng.device)
    return lambda obs, epsilon, seed, t, env_offset, out: eng.act_rows_dist(obs, head, epsilon, seed, t, env_offset=env_offset,
                                                                           q=q, out=out)


def _dist_learn(trainer, eng):
    B, o, head = trainer.batch_size, trainer.optimizer, trainer._dist_head()

    def learn(replay, seed, draw):
        hp = o.hyper(trainer.gamma, 0.0, 1.0 / B)
        eng.dist_learn_sampled(hp, *replay.arrays(), len(replay), B, seed, draw, head)
        o.step_count = hp.step
    return learn


# ---- IQN: its own engine -------------------------------------------------------------------------------------------------
def _iqn_guard(trainer, loop):
    cls = type(trainer)
    # train_online's guard (online.fast_iqn_ok) without its single-robot limits: the native calls restate the class's own
    # select_action / learn / learn_on
    if cls.learn is not IQNTrainer.learn or cls.learn_on is not IQNTrainer.learn_on or \
            cls.select_action is not IQNTrainer.select_action:
        raise NotImplementedError(f"{cls.__name__} overrides learn, learn_on or select_action, which {loop}'s "
                                  "native calls do not run; use train_online(Env(...))")
    if type(trainer.q_network) is not IQNNetwork or type(trainer.target_network) is not IQNNetwork or \
            not trainer._views_intact():
        raise RuntimeError(f"{loop} needs both networks to be IQNNetwork on the trainer's flat buffers; use "
                           "train_online(Env(...))")


def _iqn_engine(trainer, n_envs):
    return trainer._native_engine(batch=max(trainer.batch_size, min(n_envs, MAX_CHUNK)))


def _iqn_act(trainer, eng, n_envs, constrained=True):
    K = trainer.num_quantiles_n_policy
    q = torch.empty(n_envs, trainer.action_size, dtype=torch.float32, device=eng.device)
    return lambda obs, epsilon, seed, t, env_offset, out: eng.act_rows(obs, K, epsilon, seed, t, env_offset=env_offset, q=q, out=out)


def _iqn_learn(trainer, eng):
    B, o = trainer.batch_size, trainer.optimizer
    n_cur, n_tgt = trainer.num_quantiles_n_prime_loss, trainer.num_quantiles_n_double_prime_loss

    def learn(replay, seed, draw):
        g = o.param_groups[0]
        hp = eng.hyper(trainer.gamma, trainer.kappa, trainer.max_norm, o.step_count + 1, g["lr"], g["betas"], g["eps"])
        eng.learn_sampled(hp, *replay.arrays(), len(replay), B, seed, draw, n_cur, n_tgt)
        o.step_count = hp.step                   # after the call: a refused one leaves the step number with the moments
    return learn


# ---- BCQ: an act call, no online learn step ------------------------------------------------------------------------------
def _bcq_act(trainer, eng, n_envs, constrained=True):
    q = torch.empty(n_envs, trainer.action_size, dtype=torch.float32, device=eng.device)
    scratch = dict(q=q, logits=torch.empty_like(q)) if constrained else dict(q=q)
    return lambda obs, epsilon, seed, t, env_offset, out: trainer.act_rows(
        obs, epsilon, seed, t, env_offset=env_offset, constrained=constrained, out=out, **scratch)


# ---- the table -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Family:
    """What differs between the trainer families in `_run`, `batched_act` and their messages."""
    takes: type                               # the trainers it takes (family_of: the first family in FAMILIES that does)
    act: Callable                             # (trainer, eng, n_envs, constrained) -> act(obs, epsilon, seed, t, env_offset, out)
    engine: Callable = _qnet_engine           # (trainer, n_envs) -> the engine for n_envs robots
    loop: Optional[str] = None                # the name of its loop, for messages; None: no online loop
    others: str = ""                          # the refusal of another family's trainer, after "{loop} "; {name}: its class
    guard: Callable = _no_exchange            # (trainer, loop): the refusals beyond the class
    replay: Callable = _new_replay            # (trainer, sim, eng, replay) -> the replay to train into, checked
    starts: Callable = lambda trainer: None   # (trainer) -> the default learning_starts; None: training_learning_step
    prepare: Callable = _keep_replay          # (trainer, replay): the last checks, then what a run leaves on the trainer
    learn: Optional[Callable] = None          # (trainer, eng) -> learn(replay, seed, draw)
    extras: Callable = lambda replay: {}      # (replay) -> {result key: (1,) device tensor}, appended to the one read-back


PER = Family(PERTrainer, _plain_act, loop="train_vectorized_per",
             others="is PERTrainer's loop; {name} has train_vectorized or train_online(Env(...))",
             replay=_per_memory, prepare=_per_prepare, learn=_per_learn,
             extras=lambda mem: dict(total_priority=mem.tree[:1]))
BCQ = Family(BCQTrainer, _bcq_act)
PLAIN = Family(CQLTrainer, _plain_act, loop="train_vectorized",
               others="covers the plain-Q trainers (CQL, DQN, Double DQN, Dueling); {name} runs in this task through "
                      "train_online(Env(...)) (porl_amd.env.Env, the single-robot form of the same simulator)",
               learn=_plain_learn)
DIST = Family(DistTrainerBase, _dist_act, loop="train_vectorized_dist",
              others="is the loop of C51Trainer and QRDQNTrainer; {name} has train_vectorized, train_vectorized_per or "
                     "train_online(Env(...))",
              guard=_dist_guard, starts=lambda trainer: trainer.batch_size if trainer._online_threshold == "batch" else None,
              learn=_dist_learn)
IQN = Family(IQNTrainer, _iqn_act, engine=_iqn_engine, loop="train_vectorized_iqn",
             others="is the loop of IQNTrainer; {name} has train_vectorized, train_vectorized_per, train_vectorized_dist or "
                    "train_online(Env(...))",
             guard=_iqn_guard, learn=_iqn_learn)
FAMILIES = (PER, BCQ, PLAIN, DIST, IQN)       # PER and BCQ before plain Q: they subclass CQLTrainer


def family_of(cls):
    """The family of trainer class `cls`, or None."""
    return next((fam for fam in FAMILIES if issubclass(cls, fam.takes)), None)


# ---- the loop ------------------------------------------------------------------------------------------------------------
def _run(trainer, fam, sim, n_steps, replay, learn_per_step, learning_starts, block, seed):
    """`n_steps` iterations of act -> step -> learn (module docstring) for a trainer of family `fam`.  The order of the
    set-up is fixed: nothing is touched before the family refusal (so `sim` may be anything there), and a call refused up to
    check_starts leaves the trainer's counters and `device_replay`, the optimizer's step count, the simulator and the replay
    as they were."""
    if family_of(type(trainer)) is not fam:
        raise NotImplementedError(f"{fam.loop} " + fam.others.format(name=type(trainer).__name__))
    fam.guard(trainer, fam.loop)
    N_ = sim.n_envs
    eng = fam.engine(trainer, N_)
    check_sim(eng, sim, n_steps, block, learn_per_step, fam.loop, n_actions=trainer.action_size)
    replay = fam.replay(trainer, sim, eng, replay)
    starts = fam.starts(trainer) if learning_starts is None else learning_starts
    starts = check_starts(trainer, starts, replay.capacity)
    fam.prepare(trainer, replay)
    if hasattr(eng, "_ensure_bound"):
        eng._ensure_bound()
    if bool((sim.counters[:, 2] & 0xff != 0).any()):                 # before the loop: robots that are not running
        sim.reset()
    act, learn = fam.act(trainer, eng, N_), fam.learn(trainer, eng)
    actions = torch.empty(N_, dtype=torch.int64, device=eng.device)
    loss_log = torch.zeros(max(1, n_steps * learn_per_step), dtype=torch.float32, device=eng.device)
    n_learn, draw = 0, None
    for _ in range(n_steps):
        t = trainer._vec_steps = getattr(trainer, "_vec_steps", 0)
        act(sim.obs, trainer.epsilon, seed, t, sim.env_offset, actions)
        sim.step(actions, replay=replay)
        if len(replay) >= starts:
            for _k in range(learn_per_step):
                if draw is None:                                      # read at the first learn step: a run without one makes no counter
                    draw = draw_count(trainer)
                learn(replay, seed, draw)
                trainer._draws = draw = draw + 1
                loss_log[n_learn:n_learn + 1].copy_(eng.stats[:1])
                n_learn += 1
        end_of_step(trainer, t, block)                                # a block ends: the reference's per-episode schedule
    extras = fam.extras(replay)
    host = torch.cat([loss_log[:n_learn].double(), sim.tallies.sum(0), *extras.values()]).cpu().numpy()      # the one read-back
    out = dict(losses=host[:n_learn].astype("float32"), tallies=host[n_learn:n_learn + 4], transitions=N_ * n_steps,
               learn_steps=n_learn)
    out.update((key, float(x)) for key, x in zip(extras, host[n_learn + 4:]))
    return out


def train_vectorized(trainer, sim, n_steps, replay=None, learn_per_step=1, learning_starts=None, block=32, seed=0):
    """Run `n_steps` iterations of act -> step -> learn (module docstring) with `sim`, a DiscreteLidarNavSim with
    auto_reset=True whose observation and action count are the trainer's.  `replay`: a DeviceReplay (default: one of the
    trainer's replay capacity, kept as `trainer.device_replay`); `learning_starts` defaults to the trainer's
    training_learning_step, and is never below batch_size.  `seed` keys the exploration draws (with sim.env_offset + i
    and the act-step) and the minibatch draws.  Returns, after the one read-back, a dict: losses (numpy, one mean loss per
    learn step), tallies (numpy (4,): sim.tallies summed over robots — episodes, sum of returns, goals, hits), transitions,
    learn_steps.  Plain-Q trainers only: every other family's trainer raises NotImplementedError."""
    return _run(trainer, PLAIN, sim, n_steps, replay, learn_per_step, learning_starts, block, seed)


def train_vectorized_per(trainer, sim, n_steps, learn_per_step=1, learning_starts=None, block=32, seed=0):
    """`train_vectorized` for a PERTrainer, writing into `trainer.memory`.  `seed` keys the exploration draws and the
    stratified sample (apart from each other by the sampler's stream tag).  The result has total_priority (the tree's root)
    as well."""
    return _run(trainer, PER, sim, n_steps, None, learn_per_step, learning_starts, block, seed)


def train_vectorized_dist(trainer, sim, n_steps, replay=None, learn_per_step=1, learning_starts=None, block=32, seed=0):
    """`train_vectorized` for a C51Trainer or QRDQNTrainer; `learning_starts` defaults to the threshold of the trainer's own
    train_online."""
    return _run(trainer, DIST, sim, n_steps, replay, learn_per_step, learning_starts, block, seed)


def train_vectorized_iqn(trainer, sim, n_steps, replay=None, learn_per_step=1, learning_starts=None, block=32, seed=0):
    """`train_vectorized` for an IQNTrainer; `seed` keys the fractions as well."""
    return _run(trainer, IQN, sim, n_steps, replay, learn_per_step, learning_starts, block, seed)
