"""`train_vectorized_iqn`: IQNTrainer (train/iqn_trainer.py) in the discrete lidar task with N robots per step and no host
synchronisation inside the loop — `train_vectorized` (train/vector_online.py) for the trainer on the IQN engine.

One iteration, all on the current stream:
  act      IqnEngine.act_rows on `sim.obs` with num_quantiles_n_policy fractions per robot (porl_iqn_act_rows): per chunk of
           the engine's max_batch robots one staging launch (states and the fractions of the keyed stream, csrc/iqn_vector.hpp),
           the feature layers, the mix, the value layers and one wave per robot that turns its K x A quantile values into A
           means and an epsilon-greedy action — means in the order the learn step ranks the next state's actions by, so
           acting and bootstrapping agree; the actions stay on the device and the values never leave the workspace;
  step     DiscreteLidarNavSim.step(actions, replay=...) — every transition straight into the replay arrays (porl_nav_dstep);
  learn    `learn_per_step` steps once len(replay) >= learning_starts: IqnEngine.learn_sampled, the trainer's learn from one
           native call whose gather launch draws the minibatch and whose fractions tau' and tau'' come from the keyed
           stream (porl_iqn_learn_sampled), and the mean loss copied device-to-device into a loss log.

Epsilon and the target network follow `train_vectorized`'s block schedule, the counters `_vec_steps` / `_draws` live on the
trainer so a second call continues the first, and nothing is read back before the end.  The fractions are not
torch.rand's: robot `sim.env_offset + i` at act-step t and minibatch row b of learn-draw d own fixed elements of the stream
keyed by `seed`, so a run does not depend on torch's generator, on chunking, or on how robots are split over simulators.

`learning_starts=None` is the threshold of the trainer's own `train_online`: training_learning_step.
"""
from __future__ import annotations

import torch

from ..buffer.device_replay import DeviceReplay
from .vector_online import check_sim, check_starts, end_of_step

MAX_CHUNK = 1024          # robots per forward chunk: the engine's max_batch is max(batch_size, min(n_envs, MAX_CHUNK))


def _refuse(trainer):
    from ..net.iqn_network import IQNNetwork
    from .iqn_trainer import IQNTrainer
    if not isinstance(trainer, IQNTrainer):
        raise NotImplementedError(f"train_vectorized_iqn is the loop of IQNTrainer; {type(trainer).__name__} has "
                                  "train_vectorized, train_vectorized_per, train_vectorized_dist or train_online(Env(...))")
    cls = type(trainer)
    # train_online's guard (online.fast_iqn_ok) without its single-robot limits: the native calls restate the class's own
    # select_action / learn / learn_on
    if cls.learn is not IQNTrainer.learn or cls.learn_on is not IQNTrainer.learn_on or \
            cls.select_action is not IQNTrainer.select_action:
        raise NotImplementedError(f"{cls.__name__} overrides learn, learn_on or select_action, which train_vectorized_iqn's "
                                  "native calls do not run; use train_online(Env(...))")
    if type(trainer.q_network) is not IQNNetwork or type(trainer.target_network) is not IQNNetwork or \
            not trainer._views_intact():
        raise RuntimeError("train_vectorized_iqn needs both networks to be IQNNetwork on the trainer's flat buffers; use "
                           "train_online(Env(...))")


def train_vectorized_iqn(trainer, sim, n_steps, replay=None, learn_per_step=1, learning_starts=None, block=32, seed=0):
    """Run `n_steps` iterations of act -> step -> learn (module docstring) with `sim`, a DiscreteLidarNavSim with
    auto_reset=True whose observation and action count are the trainer's.  `replay`: a DeviceReplay (default: one of the
    trainer's replay capacity, kept as `trainer.device_replay`).  `seed` keys the exploration draws, the fractions and the
    minibatch draws.  Returns, after the one read-back, the dict of `train_vectorized`: losses, tallies, transitions,
    learn_steps."""
    _refuse(trainer)
    N_, S, B = sim.n_envs, sim.obs_dim, trainer.batch_size
    eng = trainer._native_engine(batch=max(B, min(N_, MAX_CHUNK)))
    check_sim(eng, sim, n_steps, block, learn_per_step, "train_vectorized_iqn")
    if replay is None:
        replay = getattr(trainer, "device_replay", None)
        if replay is None:
            replay = DeviceReplay(max(int(getattr(trainer.replay_buffer, "capacity", 100000)), N_), S, eng.device)
    starts = check_starts(trainer, learning_starts, replay.capacity)
    trainer.device_replay = replay
    if bool((sim.counters[:, 2] & 0xff != 0).any()):                 # before the loop: robots that are not running
        sim.reset()
    dev = eng.device
    K, n_cur, n_tgt = trainer.num_quantiles_n_policy, trainer.num_quantiles_n_prime_loss, trainer.num_quantiles_n_double_prime_loss
    q = torch.empty(N_, trainer.action_size, dtype=torch.float32, device=dev)
    actions = torch.empty(N_, dtype=torch.int64, device=dev)
    loss_log = torch.zeros(max(1, n_steps * learn_per_step), dtype=torch.float32, device=dev)
    o = trainer.optimizer
    n_learn = 0
    for _ in range(n_steps):
        t = trainer._vec_steps = getattr(trainer, "_vec_steps", 0)
        eng.act_rows(sim.obs, K, trainer.epsilon, seed, t, env_offset=sim.env_offset, q=q, out=actions)
        sim.step(actions, replay=replay)
        if len(replay) >= starts:
            for _k in range(learn_per_step):
                trainer._draws = getattr(trainer, "_draws", 0)
                g = o.param_groups[0]
                hp = eng.hyper(trainer.gamma, trainer.kappa, trainer.max_norm, o.step_count + 1, g["lr"], g["betas"], g["eps"])
                eng.learn_sampled(hp, *replay.arrays(), len(replay), B, seed, trainer._draws, n_cur, n_tgt)
                o.step_count = hp.step               # after the call: a refused one leaves the step number with the moments
                trainer._draws += 1
                loss_log[n_learn:n_learn + 1].copy_(eng.stats[:1])
                n_learn += 1
        end_of_step(trainer, t, block)
    host = torch.cat([loss_log[:n_learn].double(), sim.tallies.sum(0)]).cpu().numpy()      # the one read-back
    return dict(losses=host[:n_learn].astype("float32"), tallies=host[n_learn:], transitions=N_ * n_steps, learn_steps=n_learn)
