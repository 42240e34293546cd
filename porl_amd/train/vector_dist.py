"""`train_vectorized_dist`: C51Trainer and QRDQNTrainer (train/dist_trainer.py) in the discrete lidar task with N robots per
step and no host synchronisation inside the loop — `train_vectorized` (train/vector_online.py) for the two distributional
trainers on the Q-network engine.

One iteration, all on the current stream:
  act      QnetEngine.act_rows_dist on `sim.obs` with the trainer's `_dist_head()` (porl_qnet_act_rows_dist): the batched
           forward, then one wave per robot turns its A x n_sub quantiles / atom logits into A values and an epsilon-greedy
           action (csrc/dist_act.hpp) — values in the order the loss heads rank the next state's actions by, so acting and
           bootstrapping agree; the actions stay on the device and the outputs never leave the workspace;
  step     DiscreteLidarNavSim.step(actions, replay=...) — every transition straight into the replay arrays (porl_nav_dstep);
  learn    `learn_per_step` steps once len(replay) >= learning_starts: QnetEngine.dist_learn_sampled, the trainer's learn_on
           from one native call whose gather launch draws the minibatch (porl_qnet_dist_learn_sampled), and the mean loss
           copied device-to-device into a loss log.

Epsilon and the target network follow `train_vectorized`'s block schedule, the counters `_vec_steps` / `_draws` live on the
trainer so a second call continues the first, and nothing is read back before the end.

`learning_starts=None` is the threshold of the trainer's own `train_online`: batch_size for C51 (c51_trainer.py:205),
training_learning_step for QR-DQN (dqn_trainer.py:148).

`train_vectorized(qr, ...)` still refuses a distributional trainer (its message is pinned by a test); the entry points can be
folded once that test may move.  IQN has its own engine and its own loop, `train_vectorized_iqn`
(train/vector_iqn.py); BCQ is offline.
"""
from __future__ import annotations

import torch

from ..buffer.device_replay import DeviceReplay
from .vector_online import check_sim, check_starts, end_of_step


def _refuse(trainer):
    from .dist_trainer import DistTrainerBase
    if not isinstance(trainer, DistTrainerBase):
        raise NotImplementedError(f"train_vectorized_dist is the loop of C51Trainer and QRDQNTrainer; {type(trainer).__name__} "
                                  "has train_vectorized, train_vectorized_per or train_online(Env(...))")
    if trainer._exchange.active:
        raise NotImplementedError("train_vectorized_dist has no gradient exchange; use train_online(Env(...)) per rank")
    cls = type(trainer)
    # train_online's guard: the native calls restate the class's own select_action / learn_on
    if cls.learn is not DistTrainerBase.learn or cls._rows_for is None or cls._rows_for is not cls.learn_on or \
            cls._act_for is None or cls._act_for is not cls.select_action:
        raise NotImplementedError(f"{cls.__name__} overrides learn, learn_on or select_action, which train_vectorized_dist's "
                                  "native calls do not run; use train_online(Env(...))")


def train_vectorized_dist(trainer, sim, n_steps, replay=None, learn_per_step=1, learning_starts=None, block=32, seed=0):
    """Run `n_steps` iterations of act -> step -> learn (module docstring) with `sim`, a DiscreteLidarNavSim with
    auto_reset=True whose observation and action count are the trainer's.  `replay`: a DeviceReplay (default: one of the
    trainer's replay capacity, kept as `trainer.device_replay`).  `seed` keys the exploration draws and the minibatch
    draws.  Returns, after the one read-back, the dict of `train_vectorized`: losses, tallies, transitions, learn_steps."""
    _refuse(trainer)
    eng = trainer._engine
    N_, S, B = sim.n_envs, sim.obs_dim, trainer.batch_size
    check_sim(eng, sim, n_steps, block, learn_per_step, "train_vectorized_dist", n_actions=trainer.action_size)
    if replay is None:
        replay = getattr(trainer, "device_replay", None)
        if replay is None:
            replay = DeviceReplay(max(int(getattr(trainer.replay_buffer, "capacity", 100000)), N_), S, eng.device)
    if learning_starts is None and trainer._online_threshold == "batch":
        learning_starts = B
    starts = check_starts(trainer, learning_starts, replay.capacity)
    trainer.device_replay = replay
    eng._ensure_bound()
    if bool((sim.counters[:, 2] & 0xff != 0).any()):                 # before the loop: robots that are not running
        sim.reset()
    dev = eng.device
    head = trainer._dist_head()
    q = torch.empty(N_, trainer.action_size, dtype=torch.float32, device=dev)
    actions = torch.empty(N_, dtype=torch.int64, device=dev)
    loss_log = torch.zeros(max(1, n_steps * learn_per_step), dtype=torch.float32, device=dev)
    n_learn = 0
    for _ in range(n_steps):
        t = trainer._vec_steps = getattr(trainer, "_vec_steps", 0)
        eng.act_rows_dist(sim.obs, head, trainer.epsilon, seed, t, env_offset=sim.env_offset, q=q, out=actions)
        sim.step(actions, replay=replay)
        if len(replay) >= starts:
            for _k in range(learn_per_step):
                trainer._draws = getattr(trainer, "_draws", 0)
                hp = trainer.optimizer.hyper(trainer.gamma, 0.0, 1.0 / B)
                eng.dist_learn_sampled(hp, *replay.arrays(), len(replay), B, seed, trainer._draws, head)
                trainer.optimizer.step_count = hp.step
                trainer._draws += 1
                loss_log[n_learn:n_learn + 1].copy_(eng.stats[:1])
                n_learn += 1
        end_of_step(trainer, t, block)
    host = torch.cat([loss_log[:n_learn].double(), sim.tallies.sum(0)]).cpu().numpy()      # the one read-back
    return dict(losses=host[:n_learn].astype("float32"), tallies=host[n_learn:], transitions=N_ * n_steps, learn_steps=n_learn)
