#!/usr/bin/env python3
"""Golden fixtures of train_online (tests/golden/online_*.npz).  TEST INFRASTRUCTURE — runs only where the reference
implementation is importable (CPU); its output, small .npz data files, is all that travels.

Runs the reference's DQNTrainer.train_online (src/porl/train/dqn_trainer.py:119-180), DDQNTrainer.train_online (the
same loop, ddqn_trainer.py's learn) and C51Trainer.train_online (c51_trainer.py:176-225) as unbound methods on
hand-built objects (like oracle/gen_golden.py:gen_dqn), on tests/helpers/online_env.py:ToyEnv with a recording logger.
Recorded: initial weights, the action sequence, the smallest top-2 Q gap met on a greedy step, rewards_history, the
logged losses, the final epsilon, the final online / target parameters and the replay buffer's contents.

Usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_online.py </dev/null
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

# shared by the generator and tests/test_online_gpu.py (stored in each fixture's `meta`)
S, A, EPISODES, MAX_STEPS, THRESHOLD, BATCH, TARGET_FREQ, CAPACITY = 8, 4, 4, 30, 32, 32, 2, 1000
EPS, EPS_MIN, EPS_DECAY, GAMMA = 1.0, 0.05, 0.5, 0.99


def _common(t, dev):
    from porl.buffer.replaybuffer import ReplayBuffer
    t.state_size, t.action_size, t.device = S, A, dev
    t.gamma, t.epsilon, t.epsilon_min, t.epsilon_decay = GAMMA, EPS, EPS_MIN, EPS_DECAY
    t.update_target_freq, t.training_learning_step, t.batch_size = TARGET_FREQ, THRESHOLD, BATCH
    t.replay_buffer = ReplayBuffer(CAPACITY, (S,), dev)
    t.logger = RecordingLogger()


def gen(name, kind, seed_model, seed_env, seed_np, hidden=(48, 40), atoms=21, v_min=-3.0, v_max=3.0):
    _stub_cql_imports()
    from porl.net.q_network import QNetwork
    from porl.net.categorical_q_network import CategoricalQNetwork
    from porl.train.dqn_trainer import DQNTrainer
    from porl.train.ddqn_trainer import DDQNTrainer
    from porl.train.c51_trainer import C51Trainer
    cls = dict(dqn=DQNTrainer, ddqn=DDQNTrainer, c51=C51Trainer)[kind]
    dev = torch.device("cpu")
    torch.manual_seed(seed_model)
    t = object.__new__(cls)
    if kind == "c51":
        t.q_network = CategoricalQNetwork(S, A, atoms, v_min, v_max, hidden_sizes=list(hidden))
        t.target_network = CategoricalQNetwork(S, A, atoms, v_min, v_max, hidden_sizes=list(hidden))
        t.atom_size, t.v_min, t.v_max = atoms, v_min, v_max
        t.delta_z = (v_max - v_min) / (atoms - 1)
        t.support = torch.linspace(v_min, v_max, atoms)
    else:
        t.q_network, t.target_network = QNetwork(S, A), QNetwork(S, A)
    t.target_network.load_state_dict(t.q_network.state_dict())
    t.optimizer = torch.optim.Adam(t.q_network.parameters(), lr=0.0005)
    _common(t, dev)
    out = {"meta": np.array([S, A, EPISODES, MAX_STEPS, THRESHOLD, BATCH, TARGET_FREQ, CAPACITY, seed_env, seed_np, atoms]),
           "eps": np.array([EPS, EPS_MIN, EPS_DECAY, GAMMA, v_min, v_max], dtype=np.float64),
           "hidden": np.array(hidden if kind == "c51" else (64, 128, 64))}
    out.update(pack("init/", sd_np(t.q_network)))
    # the smallest top-2 gap of the Q values a greedy step chose from (batch-1 forwards are the greedy ones)
    gaps = []

    def hook(mod, inp, o):
        if o.shape[0] == 1:
            q = o.detach()
            if kind == "c51":
                q = (q.exp() * t.support).sum(-1)
            v = torch.sort(q.reshape(-1), descending=True).values
            gaps.append(float(v[0] - v[1]))
    t.q_network.register_forward_hook(hook)
    env = ToyEnv(seed=seed_env)
    np.random.seed(seed_np)
    with contextlib.redirect_stdout(io.StringIO()):
        rewards = cls.train_online(t, env, num_episodes=EPISODES, max_steps=MAX_STEPS)
    losses = [c[4] for c in t.logger.calls if c[0] == "log_step" and c[4] is not None]
    out["actions"] = np.array(env.actions, dtype=np.int64)
    out["ends"] = np.array([e == "terminated" for e in env.ends])
    out["min_gap"] = np.float64(min(gaps))
    out["n_greedy"] = np.int64(len(gaps))
    out["rewards_history"] = np.array(rewards, dtype=np.float64)
    out["losses"] = np.array(losses, dtype=np.float64)
    out["final_epsilon"] = np.float64(t.epsilon)
    # the logger's call sequence without the loss values: (method, episode, step, has loss)
    out["log_calls"] = np.array([[0, c[1], c[2], c[4] is not None] if c[0] == "log_step" else [1, c[1], -1, 0]
                                 for c in t.logger.calls if c[0] in ("log_step", "log_episode")], dtype=np.int64)
    out.update(pack("final/", sd_np(t.q_network)))
    out.update(pack("final_target/", sd_np(t.target_network)))
    rb = t.replay_buffer
    n = rb.size
    for k in ("states", "actions", "rewards", "next_states", "dones"):
        out["buf/" + k] = getattr(rb, k)[:n].copy()
    out["buf/position"] = np.int64(rb.position)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: {len(env.actions)} steps, {len(gaps)} greedy (min gap {min(gaps):.4g}), {len(losses)} losses, "
          f"ends {env.ends}, rewards {[round(r, 3) for r in rewards]}")


if __name__ == "__main__":
    gen("online_dqn_s8_a4", "dqn", seed_model=16, seed_env=26, seed_np=16)
    gen("online_ddqn_s8_a4", "ddqn", seed_model=12, seed_env=4, seed_np=6)
    gen("online_c51_s8_a4", "c51", seed_model=17, seed_env=17, seed_np=17)
