"""`train_vectorized_per`: PERTrainer (Double DQN with prioritized replay, dqn_per_trainer.py) in the discrete lidar task
with N robots per step and no host synchronisation inside the loop — `train_vectorized` (train/vector_online.py) for the one
trainer whose replay is a sum tree.

One iteration, all on the current stream:
  act      QnetEngine.act_rows on `sim.obs` (porl_qnet_act_rows); the actions stay on the device;
  step     DiscreteLidarNavSim.step(actions, replay=trainer.memory): one launch writes every robot's transition into the
           memory's store (porl_nav_dstep), one launch gives the N new leaves the priority of a new row and recomputes their
           ancestors (PrioritizedReplayBuffer.advance -> porl_per_fill_range);
  learn    `learn_per_step` steps once len(memory) >= learning_starts, each
             memory.sample_slots_keyed(B, seed, draw)   tree walk, weights and their mean, the uniforms drawn in the kernel
             engine.learn_indexed(..., slots, variant)  the weighted Double-DQN step on the store's rows, |TD| out — with
                                                        PERTrainer.learn's choice between per_sample_weights and the
                                                        reference's broadcast (mean weight)
             memory.update_priorities_device(tree_idx, |TD|)
           and the mean loss copied device-to-device into a loss log.
On a network the one-launch step kernel takes, that is 6 launches per iteration with one learn step (forward + select, step,
fill, sample, learn, write-back) and the loss copy; a wider network adds its layers' launches to act and learn.

Epsilon and the target network follow `train_vectorized`'s block schedule, the counters `_vec_steps` / `_draws` live on the
trainer so a second call continues the first, and nothing is read back before the end.

`PERTrainer.train_vectorized` still refuses (its message is pinned by a test); the two entry points can be folded once that
test may move.
"""
from __future__ import annotations

import torch

from .. import _native as N
from .vector_online import check_sim, check_starts, end_of_step


def train_vectorized_per(trainer, sim, n_steps, learn_per_step=1, learning_starts=None, block=32, seed=0):
    """Run `n_steps` iterations of act -> step -> learn (module docstring) with `sim`, a DiscreteLidarNavSim with
    auto_reset=True whose observation and action count are the trainer's, writing into `trainer.memory`.  `learning_starts`
    defaults to the trainer's training_learning_step and is never below batch_size.  `seed` keys the exploration draws and
    the stratified sample (apart from each other by the sampler's stream tag).  Returns, after the one read-back, the dict
    of `train_vectorized` — losses, tallies, transitions, learn_steps — plus total_priority (the tree's root)."""
    from .dqn_per_trainer import PERTrainer
    if not isinstance(trainer, PERTrainer):
        raise NotImplementedError(f"train_vectorized_per is PERTrainer's loop; {type(trainer).__name__} has train_vectorized "
                                  "or train_online(Env(...))")
    if trainer._exchange.active:
        raise NotImplementedError("train_vectorized_per has no gradient exchange; use train_online(Env(...)) per rank")
    eng, mem = trainer._engine, trainer.memory
    N_ = sim.n_envs
    check_sim(eng, sim, n_steps, block, learn_per_step, "train_vectorized_per")
    if mem.tree.device != eng.device or mem.state_dim != sim.obs_dim:
        raise ValueError(f"memory: need rows of {sim.obs_dim} floats on {eng.device}")
    if N_ > mem.capacity:
        raise ValueError(f"{N_} robots > memory capacity {mem.capacity}: two robots would share a slot")
    B = trainer.batch_size
    starts = check_starts(trainer, learning_starts, mem.capacity)
    if B > trainer._td_abs.numel():
        raise ValueError(f"batch_size {B} > the trainer's |TD| buffer of {trainer._td_abs.numel()}")
    eng._ensure_bound()
    if bool((sim.counters[:, 2] & 0xff != 0).any()):                 # before the loop: robots that are not running
        sim.reset()
    mem.priority_for_new = trainer.max_initial_priority
    dev = eng.device
    q = torch.empty(N_, eng.cfg.n_actions, dtype=torch.float32, device=dev)
    actions = torch.empty(N_, dtype=torch.int64, device=dev)
    loss_log = torch.zeros(max(1, n_steps * learn_per_step), dtype=torch.float32, device=dev)
    td_abs = trainer._td_abs[:B]
    rows = mem.arrays()
    n_learn = 0
    for _ in range(n_steps):
        t = trainer._vec_steps = getattr(trainer, "_vec_steps", 0)
        eng.act_rows(sim.obs, trainer.epsilon, seed, t, env_offset=sim.env_offset, q=q, out=actions)
        sim.step(actions, replay=mem)
        if len(mem) >= starts:
            for _k in range(learn_per_step):
                trainer._draws = getattr(trainer, "_draws", 0)
                slots, is_w, wmean, tree_idx = mem.sample_slots_keyed(B, seed, trainer._draws)
                hp = trainer.optimizer.hyper(trainer.gamma, 0.0, 1.0 / B)
                if trainer.per_sample_weights:
                    var = N.QnetVariant(1, is_w.data_ptr(), None, td_abs.data_ptr())
                else:                                                 # the reference's (B,1)*(B,) broadcast: mean(w)*mean(td^2)
                    var = N.QnetVariant(1, None, wmean.data_ptr(), td_abs.data_ptr())
                eng.learn_indexed(hp, *rows, slots, variant=var)
                trainer.optimizer.step_count = hp.step
                mem.update_priorities_device(tree_idx, td_abs)
                trainer._draws += 1
                loss_log[n_learn:n_learn + 1].copy_(eng.stats[:1])
                n_learn += 1
        end_of_step(trainer, t, block)
    host = torch.cat([loss_log[:n_learn].double(), sim.tallies.sum(0), mem.tree[:1]]).cpu().numpy()    # the one read-back
    return dict(losses=host[:n_learn].astype("float32"), tallies=host[n_learn:-1], transitions=N_ * n_steps,
                learn_steps=n_learn, total_priority=float(host[-1]))
