#!/usr/bin/env python3
"""Golden fixture of BCQTrainer.train(policy=bcq_learn) (tests/golden/online_bcq_s8_a4.npz).  TEST INFRASTRUCTURE — runs
only where the reference implementation is importable (CPU); its output, one small .npz data file, is all that travels.

A reference BCQTrainer is built by hand (like oracle/gen_golden.py:gen_bcq; its constructor needs gymnasium) on
tests/helpers/online_env.py:ToyEnv with a recording logger.  Then
  1. the buffer is filled with a seeded random roll-out written here (uniform random actions on a ToyEnv of its own),
  2. the reference's unmodified bcq_behavior_pretrain runs for a handful of epochs,
  3. the reference's unmodified DQNTrainer.train_online runs unbound with policy=lambda: bcq_learn(t) — the reading of
     BCQTrainer.train's `super().train(env, policy, num_episodes, max_steps)`.
Recorded: what scripts/gen_golden_online.py records, plus the behaviour policy before / after the pre-training and
  mask_mean  : mean of the behaviour mask over all learn batches,
  min_margin : smallest |p - threshold| over every behaviour probability of every learn batch,
  min_gap    : smallest top-2 gap of the Q values a greedy step chose from and of the masked target Q values
               (next_q + (mask - 1) * 1e10, the reference's fp32 arithmetic) a learn step took its argmax of.
Seeds and threshold are picked so that min_margin >= 1e-4, min_gap > 1e-3 and 0.2 < mask_mean < 0.8 (asserted below).

Usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_online_bcq.py </dev/null
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

from oracle.gen_golden import OUT, _stub_cql_imports, pack, sd_np  # noqa: E402
from helpers.online_env import RecordingLogger, ToyEnv  # noqa: E402

S, A, EPISODES, MAX_STEPS, THRESHOLD, BATCH, TARGET_FREQ, CAPACITY = 8, 4, 4, 30, 32, 32, 2, 1000
EPS, EPS_MIN, EPS_DECAY, GAMMA = 1.0, 0.05, 0.5, 0.99
PREFILL, EPOCHS = 96, 8


def rollout(rb, n, seed):
    """n transitions of uniformly random actions on a ToyEnv of its own (its generator also draws the actions)."""
    env = ToyEnv(seed=seed)
    rng = np.random.default_rng(seed + 1000)
    state, _ = env.reset()
    for _ in range(n):
        a = int(rng.integers(A))
        nxt, r, term, trunc, _ = env.step(a)
        rb.push(state, a, r, nxt, term or trunc)
        state = env.reset()[0] if (term or trunc) else nxt


def gen(name, seed_model, seed_env, seed_np, seed_data, threshold, write=True):
    _stub_cql_imports()
    from porl.buffer.replaybuffer import ReplayBuffer
    from porl.net.behavior_policy import BehaviorPolicy
    from porl.net.q_network import QNetwork
    from porl.policy.bcq import bcq_behavior_pretrain, bcq_learn
    from porl.train.bcq_trainer import BCQTrainer
    from porl.train.dqn_trainer import DQNTrainer
    dev = torch.device("cpu")
    torch.manual_seed(seed_model)
    t = object.__new__(BCQTrainer)
    t.q_network, t.target_network = QNetwork(S, A), QNetwork(S, A)
    t.target_network.load_state_dict(t.q_network.state_dict())
    t.optimizer = torch.optim.Adam(t.q_network.parameters(), lr=0.0005)
    t.behavior_policy = BehaviorPolicy(S, A)                               # bcq_trainer.py:59-62
    t.behavior_optimizer = torch.optim.Adam(t.behavior_policy.parameters(), lr=0.0005)
    t.state_size, t.action_size, t.device = S, A, dev
    t.gamma, t.epsilon, t.epsilon_min, t.epsilon_decay = GAMMA, EPS, EPS_MIN, EPS_DECAY
    t.update_target_freq, t.training_learning_step, t.batch_size = TARGET_FREQ, THRESHOLD, BATCH
    t.num_epochs, t.threshold = EPOCHS, threshold
    t.replay_buffer = ReplayBuffer(CAPACITY, (S,), dev)
    t.logger = RecordingLogger()
    rollout(t.replay_buffer, PREFILL, seed_data)
    out = {"meta": np.array([S, A, EPISODES, MAX_STEPS, THRESHOLD, BATCH, TARGET_FREQ, CAPACITY, seed_env, seed_np, PREFILL,
                             EPOCHS, seed_data]),
           "eps": np.array([EPS, EPS_MIN, EPS_DECAY, GAMMA], dtype=np.float64), "threshold": np.float64(threshold)}
    out.update(pack("init/", sd_np(t.q_network)))
    out.update(pack("init_behavior/", sd_np(t.behavior_policy)))
    rb = t.replay_buffer
    for k in ("states", "actions", "rewards", "next_states", "dones"):
        out["prefill/" + k] = getattr(rb, k)[:PREFILL].copy()
    np.random.seed(seed_np)
    with contextlib.redirect_stdout(io.StringIO()):
        bcq_behavior_pretrain(t)
    out.update(pack("behavior_after/", sd_np(t.behavior_policy)))

    gaps, learn_gaps, margins, masks, last = [], [], [], [], {}

    def q_hook(mod, inp, o):
        if o.shape[0] == 1:                                                # the greedy steps' batch-1 forwards
            v = torch.sort(o.detach().reshape(-1), descending=True).values
            gaps.append(float(v[0] - v[1]))

    def beh_hook(mod, inp, o):                                             # BehaviorPolicy.forward inside sample()
        p = o.detach()
        margins.append(float((p.double() - threshold).abs().min()))
        last["mask"] = (p > threshold).float()
        masks.append(last["mask"].numpy().copy())

    def tgt_hook(mod, inp, o):                                             # target_network(next_states) in bcq_learn
        masked = o.detach() + (last["mask"] - 1) * 1e10
        v = torch.sort(masked, dim=1, descending=True).values
        learn_gaps.append(float((v[:, 0] - v[:, 1]).min()))
    t.q_network.register_forward_hook(q_hook)
    t.behavior_policy.register_forward_hook(beh_hook)
    t.target_network.register_forward_hook(tgt_hook)
    env = ToyEnv(seed=seed_env)
    with contextlib.redirect_stdout(io.StringIO()):
        rewards = DQNTrainer.train_online(t, env, policy=lambda: bcq_learn(t), num_episodes=EPISODES, max_steps=MAX_STEPS)
    losses = [c[4] for c in t.logger.calls if c[0] == "log_step" and c[4] is not None]
    out["actions"] = np.array(env.actions, dtype=np.int64)
    out["ends"] = np.array([e == "terminated" for e in env.ends])
    out["min_gap"] = np.float64(min(gaps + learn_gaps))
    out["n_greedy"] = np.int64(len(gaps))
    out["mask_mean"] = np.float64(np.mean(masks))
    out["min_margin"] = np.float64(min(margins))
    out["rewards_history"] = np.array(rewards, dtype=np.float64)
    out["losses"] = np.array(losses, dtype=np.float64)
    out["final_epsilon"] = np.float64(t.epsilon)
    out["log_calls"] = np.array([[0, c[1], c[2], c[4] is not None] if c[0] == "log_step" else [1, c[1], -1, 0]
                                 for c in t.logger.calls if c[0] in ("log_step", "log_episode")], dtype=np.int64)
    out.update(pack("final/", sd_np(t.q_network)))
    out.update(pack("final_target/", sd_np(t.target_network)))
    n = rb.size
    for k in ("states", "actions", "rewards", "next_states", "dones"):
        out["buf/" + k] = getattr(rb, k)[:n].copy()
    out["buf/position"] = np.int64(rb.position)
    ok = float(out["min_margin"]) >= 1e-4 and float(out["min_gap"]) > 1e-3 and 0.2 < float(out["mask_mean"]) < 0.8 and \
        len(gaps) > 10 and out["ends"].any() and not out["ends"].all()
    print(f"{name}: {len(env.actions)} steps, {len(gaps)} greedy, {len(losses)} losses, min gap {float(out['min_gap']):.4g}, "
          f"min margin {float(out['min_margin']):.4g}, mask mean {float(out['mask_mean']):.3f}, ends {env.ends} -> "
          f"{'ok' if ok else 'REJECTED'}")
    if write:
        assert ok, "pick other seeds / another threshold: the fixture's conditions do not hold"
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    return ok


if __name__ == "__main__":
    gen("online_bcq_s8_a4", seed_model=38, seed_env=40, seed_np=42, seed_data=46, threshold=0.245)
