#!/usr/bin/env python3
"""Environment steps per second of DQNTrainer.train_online: the one-launch path (porl_qnet_act / ReplayBuffer.record /
in-kernel gather, porl_amd/train/online.py) against the reference loop on the same trainer (select_action + push +
learn).  Zero-cost environment, S = 8, A = 4, the default [64, 128, 64] QNetwork, batch 64, a 100 k buffer pre-filled
with 1 000 transitions so that every timed step learns.  Two action regimes, reported separately:
  greedy  : epsilon = 0 — every step acts through the network
  explore : epsilon = 1 — every step draws a random action (no forward at all)

    python scripts/bench_online.py [--steps 3000] [--warmup 300] [--trainer dqn|per|c51|qr|iqn] [--regime greedy|explore]
                                   [--no-reference-loop]

--trainer per: PERTrainer.train_online (Double DQN on prioritized replay, learns from len(memory) >= batch_size on):
the one-launch path (PrioritizedReplayBuffer.record / sample_slots / update_priorities_device around the step kernel)
against the loop on select_action + memory.add + learn, same network, batch and pre-fill.  On a tree without the PER
one-launch path both columns time the plain loop ("one_launch": false) — the figure to compare another tree's against.

--trainer c51 / qr: C51Trainer / QRDQNTrainer.train_online on the class-default [128, 128] network (51 atoms / 51
quantiles), same batch and pre-fill, every step learns: the one-launch act / record with the one-call learn step
(porl_qnet_dist_learn on the sampled rows of the mirror) against the loop on select_action + push + learn.  On a tree
without the one-call learn step the first column times act / record around the multi-launch learn() ("one_launch":
false) — the figure to compare another tree's against.

--trainer iqn: IQNTrainer.train_online on the class-default network (hidden 512, 64 cosine features, 8 / 8 / 32
fractions), same batch and pre-fill, every step learns: the native act (porl_iqn_act) / record with the one-call learn
step (porl_iqn_learn on the sampled rows of the mirror) against the loop on select_action + push + learn.  On a tree
without the native path both columns time the plain loop ("one_launch": false) — the figure to compare another tree's
against.

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from porl_amd.train import online  # noqa: E402
from porl_amd.train.dqn_trainer import DQNTrainer  # noqa: E402

S, A, B, CAP, PREFILL = 8, 4, 64, 100_000, 1000


class ZeroEnv:
    """No work per step: the same state back, a constant reward, episodes end by truncation only."""

    def __init__(self, max_len):
        self.max_len = max_len
        self.s = np.linspace(-1.0, 1.0, S, dtype=np.float32)

    def reset(self, seed=None):
        self.t = 0
        return self.s, {}

    def step(self, action):
        self.t += 1
        return self.s, 0.5, False, self.t >= self.max_len, {}

    def close(self):
        pass


class NullLogger:
    def log_step(self, *a):
        pass

    def log_episode(self, *a):
        pass

    def close(self):
        pass


def run(fast, eps, steps, warmup):
    torch.manual_seed(0)
    np.random.seed(0)
    t = DQNTrainer(S, A, 0.99, epsilon=eps, epsilon_min=eps, epsilon_decay=1.0, update_target_freq=10, device="cuda",
                   batch_size=B, transition_learning_step=B)
    t.logger = NullLogger()
    rng = np.random.default_rng(1)
    for _ in range(PREFILL):
        t.replay_buffer.push(rng.standard_normal(S).astype(np.float32), int(rng.integers(A)), float(rng.standard_normal()),
                             rng.standard_normal(S).astype(np.float32), False)
    t.replay_buffer._sync_mirror()
    orig = online.fast_ok
    assert orig(t), "the one-launch path does not apply to this trainer"
    if not fast:
        online.fast_ok = lambda trainer: False
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            t.train_online(ZeroEnv(warmup), num_episodes=1, max_steps=warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.train_online(ZeroEnv(steps), num_episodes=1, max_steps=steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    finally:
        online.fast_ok = orig
    return steps / dt


def per_one_launch(t):
    ok = getattr(online, "fast_per_ok", None)
    return bool(ok is not None and ok(t))


def run_per(fast, eps, steps, warmup):
    import random
    from porl_amd.train.dqn_per_trainer import PERTrainer
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(0)
    t = PERTrainer(S, A, 0.99, epsilon=eps, epsilon_min=eps, epsilon_decay=1.0, update_target_freq=10, device="cuda",
                   batch_size=B, capacity=CAP)
    t.logger = NullLogger()
    rng = np.random.default_rng(1)
    for _ in range(PREFILL):
        t.memory.add(float(abs(rng.standard_normal())) + 0.01, rng.standard_normal(S).astype(np.float32), int(rng.integers(A)),
                     float(rng.standard_normal()), rng.standard_normal(S).astype(np.float32), False)
    t.memory._flush()
    orig = getattr(online, "fast_per_ok", None)
    if not fast and orig is not None:
        online.fast_per_ok = lambda trainer: False
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            t.train_online(ZeroEnv(warmup), num_episodes=1, max_steps=warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.train_online(ZeroEnv(steps), num_episodes=1, max_steps=steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    finally:
        if orig is not None:
            online.fast_per_ok = orig
    return steps / dt, per_one_launch(t)


def run_dist(kind, fast, eps, steps, warmup):
    from porl_amd.train.c51_trainer import C51Trainer
    from porl_amd.train.qr_dqn_trainer import QRDQNTrainer
    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(epsilon=eps, epsilon_min=eps, epsilon_decay=1.0, update_target_freq=10, device="cuda", batch_size=B)
    t = C51Trainer(S, A, 0.99, **kw) if kind == "c51" else QRDQNTrainer(S, A, 0.99, transition_learning_step=B, **kw)
    t.logger = NullLogger()
    rng = np.random.default_rng(1)
    for _ in range(PREFILL):
        t.replay_buffer.push(rng.standard_normal(S).astype(np.float32), int(rng.integers(A)), float(rng.standard_normal()),
                             rng.standard_normal(S).astype(np.float32), False)
    t.replay_buffer._sync_mirror()
    orig = online.fast_ok
    assert orig(t), "the one-launch path does not apply to this trainer"
    one_launch = getattr(type(t), "_rows_for", None) is not None
    if not fast:
        online.fast_ok = lambda trainer: False
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            t.train_online(ZeroEnv(warmup), num_episodes=1, max_steps=warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.train_online(ZeroEnv(steps), num_episodes=1, max_steps=steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    finally:
        online.fast_ok = orig
    return steps / dt, one_launch


def run_iqn(fast, eps, steps, warmup):
    from porl_amd.train.iqn_trainer import IQNTrainer
    torch.manual_seed(0)
    np.random.seed(0)
    t = IQNTrainer(S, A, 0.99, epsilon=eps, epsilon_min=eps, epsilon_decay=1.0, update_target_freq=10, device="cuda",
                   batch_size=B, buffer_size=CAP, transition_learning_step=B)
    t.logger = NullLogger()
    rng = np.random.default_rng(1)
    for _ in range(PREFILL):
        t.replay_buffer.push(rng.standard_normal(S).astype(np.float32), int(rng.integers(A)), float(rng.standard_normal()),
                             rng.standard_normal(S).astype(np.float32), False)
    t.replay_buffer._sync_mirror()
    orig = getattr(online, "fast_iqn_ok", None)
    one_launch = bool(orig is not None and orig(t))
    if not fast and orig is not None:
        online.fast_iqn_ok = lambda trainer: False
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            t.train_online(ZeroEnv(warmup), num_episodes=1, max_steps=warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.train_online(ZeroEnv(steps), num_episodes=1, max_steps=steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
    finally:
        if orig is not None:
            online.fast_iqn_ok = orig
    return steps / dt, one_launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--trainer", choices=("dqn", "per", "c51", "qr", "iqn"), default="dqn")
    ap.add_argument("--regime", choices=("greedy", "explore", "both"), default="both")
    ap.add_argument("--no-reference-loop", action="store_true", help="time the default path only")
    a = ap.parse_args()
    dist = a.trainer in ("c51", "qr")
    out = {"metric": "train_online env steps/s", "trainer": a.trainer,
           "config": dict(S=S, A=A, hidden=[128, 128] if dist else [64, 128, 64], batch=B, capacity=CAP, steps=a.steps,
                          every_step_learns=True)}
    if a.trainer == "iqn":
        out["config"].update(hidden=512, embedding_dim=64, fractions=[8, 8, 32])
    for name, eps in (("greedy", 0.0), ("explore", 1.0)):
        if a.regime not in (name, "both"):
            continue
        if a.trainer == "per":
            fast, out["one_launch"] = run_per(True, eps, a.steps, a.warmup)
            plain = None if a.no_reference_loop else run_per(False, eps, a.steps, a.warmup)[0]
        elif a.trainer == "iqn":
            fast, out["one_launch"] = run_iqn(True, eps, a.steps, a.warmup)
            plain = None if a.no_reference_loop else run_iqn(False, eps, a.steps, a.warmup)[0]
        elif dist:
            fast, out["one_launch"] = run_dist(a.trainer, True, eps, a.steps, a.warmup)
            plain = None if a.no_reference_loop else run_dist(a.trainer, False, eps, a.steps, a.warmup)[0]
        else:
            fast = run(True, eps, a.steps, a.warmup)
            plain = None if a.no_reference_loop else run(False, eps, a.steps, a.warmup)
        out[name] = dict(fast=round(fast, 1))
        if plain is not None:
            out[name].update(reference_loop=round(plain, 1), ratio=round(fast / plain, 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
