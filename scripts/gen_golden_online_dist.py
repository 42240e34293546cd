#!/usr/bin/env python3
"""Golden fixture of QRDQNTrainer.train_online (tests/golden/online_qrdqn_s8_a4.npz).  TEST INFRASTRUCTURE — runs only
where the reference implementation is importable (CPU); its output, a small .npz data file, is all that travels.

Runs the reference's train_online (src/porl/train/dqn_trainer.py:119-180, which QRDQNTrainer inherits) with
QRDQNTrainer.learn (qr_dqn_trainer.py:97-222) and QRDQNTrainer.select_action (:224-260) as unbound methods on a
hand-built object (like scripts/gen_golden_online.py), on tests/helpers/online_env.py:ToyEnv with a recording logger:
S = 8, A = 4, 12 quantiles, hidden sizes (48, 40), kappa = 0.6 (both Huber branches occur), batch 16, learn threshold 24,
a 1000-slot ring that does not wrap.  Recorded: the keys of online_c51_s8_a4 (initial weights, the action sequence, the
smallest top-2 gap of the quantile means met on a greedy step, rewards_history, the logged losses and the log-call
sequence, the final epsilon, the final online / target parameters, the replay buffer's contents) plus `kappa`;
meta[10] is the number of quantiles.

The seeds are chosen with --scan: a run whose smallest greedy top-2 gap is at least 1e-3, so that exact action equality
with an implementation that sums in another order is meaningful.

Usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_online_dist.py [--scan N] </dev/null
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

S, A, EPISODES, MAX_STEPS, THRESHOLD, BATCH, TARGET_FREQ, CAPACITY = 8, 4, 4, 30, 24, 16, 2, 1000
EPS, EPS_MIN, EPS_DECAY, GAMMA = 1.0, 0.05, 0.5, 0.99
NQ, HIDDEN, KAPPA, LR = 12, (48, 40), 0.6, 5e-4
MIN_GAP = 1e-3


def run(seed_model, seed_env, seed_np):
    """One reference run -> the fixture's dict."""
    _stub_cql_imports()
    from porl.buffer.replaybuffer import ReplayBuffer
    from porl.net.qr_dqn_network import QRNetwork
    from porl.train.qr_dqn_trainer import QRDQNTrainer
    dev = torch.device("cpu")
    torch.manual_seed(seed_model)
    t = object.__new__(QRDQNTrainer)
    t.q_network = QRNetwork(S, A, NQ, list(HIDDEN))
    t.target_network = QRNetwork(S, A, NQ, list(HIDDEN))
    t.target_network.load_state_dict(t.q_network.state_dict())
    t.target_network.eval()
    t.optimizer = torch.optim.Adam(t.q_network.parameters(), lr=LR)
    t.num_quantiles, t.kappa = NQ, KAPPA
    i = torch.arange(0, NQ, dtype=torch.float32)
    t.tau = ((2 * i + 1) / (2 * NQ)).unsqueeze(0)
    t.state_size, t.action_size, t.device = S, A, dev
    t.gamma, t.epsilon, t.epsilon_min, t.epsilon_decay = GAMMA, EPS, EPS_MIN, EPS_DECAY
    t.update_target_freq, t.training_learning_step, t.batch_size = TARGET_FREQ, THRESHOLD, BATCH
    t.replay_buffer = ReplayBuffer(CAPACITY, (S,), dev)
    t.logger = RecordingLogger()
    out = {"meta": np.array([S, A, EPISODES, MAX_STEPS, THRESHOLD, BATCH, TARGET_FREQ, CAPACITY, seed_env, seed_np, NQ]),
           "eps": np.array([EPS, EPS_MIN, EPS_DECAY, GAMMA], dtype=np.float64),
           "kappa": np.float64(KAPPA),
           "hidden": np.array(HIDDEN)}
    out.update(pack("init/", sd_np(t.q_network)))
    # the smallest top-2 gap of the quantile means a greedy step chose from: get_mean_q_values calls forward() directly
    # (no module hook sees it), so the method is watched on the instance; batch-1 calls are the greedy ones
    gaps = []
    mean_q = t.q_network.get_mean_q_values

    def watched(x):
        q = mean_q(x)
        if q.shape[0] == 1:
            v = torch.sort(q.detach().reshape(-1), descending=True).values
            gaps.append(float(v[0] - v[1]))
        return q
    t.q_network.get_mean_q_values = watched
    env = ToyEnv(seed=seed_env)
    np.random.seed(seed_np)
    with contextlib.redirect_stdout(io.StringIO()):
        rewards = QRDQNTrainer.train_online(t, env, num_episodes=EPISODES, max_steps=MAX_STEPS)
    losses = [c[4] for c in t.logger.calls if c[0] == "log_step" and c[4] is not None]
    out["actions"] = np.array(env.actions, dtype=np.int64)
    out["ends"] = np.array([e == "terminated" for e in env.ends])
    out["min_gap"] = np.float64(min(gaps) if gaps else np.inf)
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
    return out


def gen(name, seed_model, seed_env, seed_np):
    out = run(seed_model, seed_env, seed_np)
    n = len(out["actions"])
    assert float(out["min_gap"]) >= MIN_GAP, float(out["min_gap"])
    assert len(out["losses"]) > 10 and int(out["n_greedy"]) > 10
    assert n < CAPACITY and int(out["buf/position"]) == n            # the ring is not wrapped
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: {n} steps, {int(out['n_greedy'])} greedy (min gap {float(out['min_gap']):.4g}), "
          f"{len(out['losses'])} losses, rewards {[round(r, 3) for r in out['rewards_history']]}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--scan":           # the guard values of seeds k = 0..N-1, nothing written
        for k in range(int(sys.argv[2]) if len(sys.argv) > 2 else 40):
            o = run(k, k + 1, k + 2)
            print(k, len(o["actions"]), len(o["losses"]), int(o["n_greedy"]), f"{float(o['min_gap']):.3g}")
    else:
        gen("online_qrdqn_s8_a4", seed_model=10, seed_env=11, seed_np=12)
