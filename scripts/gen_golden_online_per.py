#!/usr/bin/env python3
"""Golden fixture of PERTrainer.train_online (tests/golden/online_per_s8_a4.npz).  TEST INFRASTRUCTURE — runs only where
the reference implementation is importable (CPU); its output, a small .npz data file, is all that travels.

Runs the reference's PERTrainer.train_online (src/porl/train/dqn_per_trainer.py:127-175) as an unbound method on a
hand-built object (like scripts/gen_golden_online.py) holding PrioritizedReplayBuffer(CAP, alpha=0.6, beta_start=0.4,
beta_frames=1000) and QNetwork(8, 4), on tests/helpers/online_env.py:ToyEnv with a recording logger, under pinned
np.random / random seeds.  Recorded: initial weights, the action sequence, rewards_history, the logged losses and the
log-call sequence, the final epsilon, the final online / target parameters, the final tree with n_entries, data_pointer,
beta and frame_count, the stored transitions by slot, and three guard values that say how far the run stayed from any
decision a rounding difference could flip:
  min_gap     smallest top-2 Q gap on a greedy step
  min_margin  over every draw and every tree level |s - tree[left]| / total: the distance of any sampled index from
              flipping under a perturbation of the priorities
  n_resample  times the reference's "empty slot -> resample from the full range" branch fired (the device buffer has no
              such branch: empty leaves carry zero priority)
The ring (CAP slots) does not wrap in this run; wrapping is pinned exactly by the record-vs-add twin test.

Usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_online_per.py </dev/null
"""
from __future__ import annotations

import contextlib
import io
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

from oracle.gen_golden import OUT, _stub_cql_imports, pack, sd_np  # noqa: E402
from helpers.online_env import RecordingLogger, ToyEnv  # noqa: E402

S, A, EPISODES, MAX_STEPS, BATCH, TARGET_FREQ, CAPACITY = 8, 4, 4, 30, 16, 2, 64
EPS, EPS_MIN, EPS_DECAY, GAMMA = 1.0, 0.05, 0.5, 0.99
ALPHA, BETA_START, BETA_FRAMES = 0.6, 0.4, 1000


def run(seed_model, seed_env, seed_np, seed_random):
    """One reference run -> the fixture's dict."""
    _stub_cql_imports()
    from porl.buffer.prioritized_replay_buffer import PrioritizedReplayBuffer
    from porl.buffer.sum_tree import SumTree
    from porl.net.q_network import QNetwork
    from porl.train.dqn_per_trainer import PERTrainer
    dev = torch.device("cpu")
    torch.manual_seed(seed_model)
    t = object.__new__(PERTrainer)
    t.q_network, t.target_network = QNetwork(S, A), QNetwork(S, A)
    t.target_network.load_state_dict(t.q_network.state_dict())
    t.optimizer = torch.optim.Adam(t.q_network.parameters(), lr=0.0005)
    t.state_size, t.action_size, t.device = S, A, dev
    t.gamma, t.epsilon, t.epsilon_min, t.epsilon_decay = GAMMA, EPS, EPS_MIN, EPS_DECAY
    t.update_target_freq, t.batch_size = TARGET_FREQ, BATCH
    t.memory = PrioritizedReplayBuffer(CAPACITY, alpha=ALPHA, beta_start=BETA_START, beta_frames=BETA_FRAMES)
    t.max_initial_priority = 1.0
    t.logger = RecordingLogger()
    out = {"meta": np.array([S, A, EPISODES, MAX_STEPS, BATCH, TARGET_FREQ, CAPACITY, seed_model, seed_env, seed_np,
                             seed_random]),
           "eps": np.array([EPS, EPS_MIN, EPS_DECAY, GAMMA], dtype=np.float64),
           "per": np.array([ALPHA, BETA_START, BETA_FRAMES], dtype=np.float64)}
    out.update(pack("init/", sd_np(t.q_network)))

    gaps = []

    def hook(mod, inp, o):                                     # batch-1 forwards are the greedy steps
        if o.shape[0] == 1:
            v = torch.sort(o.detach().reshape(-1), descending=True).values
            gaps.append(float(v[0] - v[1]))
    t.q_network.register_forward_hook(hook)

    # the tree walk, watched: every comparison `s <= tree[left]` of every draw, relative to the total
    tree = t.memory.tree
    margins = []

    class Watched(SumTree):
        def _retrieve(self, idx, s):
            left = 2 * idx + 1
            if left < len(self.tree):
                margins.append(abs(s - self.tree[left]) / self.tree[0])
            return SumTree._retrieve(self, idx, s)
    tree.__class__ = Watched
    uniform_calls = [0]
    orig_uniform = random.uniform

    def uniform(a, b):
        uniform_calls[0] += 1
        return orig_uniform(a, b)

    env = ToyEnv(seed=seed_env)
    np.random.seed(seed_np)
    random.seed(seed_random)
    random.uniform = uniform
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            rewards = PERTrainer.train_online(t, env, num_episodes=EPISODES, max_steps=MAX_STEPS)
    finally:
        random.uniform = orig_uniform
    losses = [c[4] for c in t.logger.calls if c[0] == "log_step" and c[4] is not None]
    out["actions"] = np.array(env.actions, dtype=np.int64)
    out["ends"] = np.array([e == "terminated" for e in env.ends])
    out["min_gap"] = np.float64(min(gaps) if gaps else np.inf)
    out["n_greedy"] = np.int64(len(gaps))
    out["min_margin"] = np.float64(min(margins) if margins else np.inf)
    out["n_resample"] = np.int64(uniform_calls[0] - BATCH * t.memory.frame_count)
    out["rewards_history"] = np.array(rewards, dtype=np.float64)
    out["losses"] = np.array(losses, dtype=np.float64)
    out["final_epsilon"] = np.float64(t.epsilon)
    out["log_calls"] = np.array([[0, c[1], c[2], c[4] is not None] if c[0] == "log_step" else [1, c[1], -1, 0]
                                 for c in t.logger.calls if c[0] in ("log_step", "log_episode")], dtype=np.int64)
    out.update(pack("final/", sd_np(t.q_network)))
    out.update(pack("final_target/", sd_np(t.target_network)))
    out["tree"] = tree.tree.copy()
    out["n_entries"], out["data_pointer"] = np.int64(tree.n_entries), np.int64(tree.data_pointer)
    out["wrapped"] = np.bool_(len(env.actions) > CAPACITY)
    out["beta"], out["frame_count"] = np.float64(t.memory.beta), np.int64(t.memory.frame_count)
    n = tree.n_entries
    data = [tree.data[i] for i in range(n)]
    out["buf/states"] = np.stack([np.asarray(d[0], dtype=np.float32) for d in data])
    out["buf/actions"] = np.array([int(d[1]) for d in data], dtype=np.int64)
    out["buf/rewards"] = np.array([np.float32(d[2]) for d in data], dtype=np.float32)
    out["buf/next_states"] = np.stack([np.asarray(d[3], dtype=np.float32) for d in data])
    out["buf/dones"] = np.array([np.float32(d[4]) for d in data], dtype=np.float32)
    return out


def gen(name, k):
    out = run(seed_model=k, seed_env=k + 1, seed_np=k + 2, seed_random=k + 3)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: {len(out['actions'])} steps, {int(out['n_greedy'])} greedy (min gap {float(out['min_gap']):.4g}), "
          f"{len(out['losses'])} losses, min margin {float(out['min_margin']):.3g}, {int(out['n_resample'])} resamples, "
          f"wrapped {bool(out['wrapped'])}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--scan":           # the guard values of seeds k = 0..N-1, nothing written
        for k in range(int(sys.argv[2]) if len(sys.argv) > 2 else 40):
            o = run(k, k + 1, k + 2, k + 3)
            print(k, len(o["actions"]), len(o["losses"]), int(o["n_greedy"]), f"{float(o['min_gap']):.3g}",
                  f"{float(o['min_margin']):.3g}", int(o["n_resample"]), bool(o["wrapped"]))
    else:
        gen("online_per_s8_a4", 24)
