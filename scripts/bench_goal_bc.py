#!/usr/bin/env python3
"""Time of one goal-conditioned behaviour-cloning step including its minibatch load, against the only native way to get
the same update without porl_iql_bc_step: porl_iql_policy_only_step with weight_mode = 1 and alpha = 0 (weights exp(0) = 1)
on a batch that torch gathers and concatenates.

    new:  load_batch_pairs (draw + gather + stage, one launch)  ->  bc_step
    old:  sample_indices -> gather_rows -> torch.cat([s, s']) -> load_batch -> policy_only_step (alpha = 0)

Both on S = G = 60, A = 2, H = 1024, L = 2, B = 1024 by default, rows drawn from a 1 M-row device store.  The two are
alternated in one process after a warm-up; each sample is device events around `--steps` steps, and the median of
`--repeats` samples is reported, with the labelled launches of one step of each (porl_prof_*).  Prints one JSON line.

Usage:  python scripts/bench_goal_bc.py [--steps 200] [--repeats 5] [--rows 1000000] [--hidden 1024] [--batch 1024]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from porl_amd import engine as E  # noqa: E402
from porl_amd.engine import IqlEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device("cuda")
    S = G = 60
    A, L, H, B = 2, 2, a.hidden, a.batch
    W = 2 * S + 2 + A
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = torch.randn(a.rows, W, device=dev, generator=gen)
    engines = []
    for _ in range(2):
        eng = IqlEngine(S + G, A, H, L, False, False, weight_mode=1, max_batch=B, device=dev)
        eng.params_pol.copy_(0.02 * torch.randn(eng.params_pol.shape, device=dev, generator=gen))
        eng._ensure_bound()
        engines.append(eng)
    new, old = engines
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    packed = torch.empty(B, W, device=dev)
    count = [0, 0]

    def step_new():
        count[0] += 1
        new.load_batch_pairs(rows, B, S, A, S + 1, G, seed=7, step=count[0])
        new.bc_step(new.hyper(inv_batch=1.0 / B, policy_step=count[0]))

    def step_old():
        count[1] += 1
        E.sample_indices(a.rows, B, 7, count[1], out=idx)
        E.gather_rows(rows, idx, out=packed)
        s, sp = packed[:, :S], packed[:, S + 1:2 * S + 1]
        x = torch.cat([s, sp], dim=1)
        old.load_batch(x, x, packed[:, S], packed[:, 2 * S + 1], packed[:, 2 * S + 2:])
        old.policy_only(old.hyper(alpha=0.0, inv_batch=1.0 / B, policy_step=count[1]))

    def launches(fn):
        E.prof_enable(True)
        try:
            fn()
            return {p["name"]: p["launches"] for p in E.prof_read(512) if p["launches"]}
        finally:
            E.prof_enable(False)

    def sample(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / a.steps            # microseconds per step

    for _ in range(a.warmup):
        step_new()
        step_old()
    torch.cuda.synchronize()
    times = {"new": [], "old": []}
    for _ in range(a.repeats):
        times["new"].append(sample(step_new))
        times["old"].append(sample(step_old))
    prof = {"new": launches(step_new), "old": launches(step_old)}
    out = dict(S=S, G=G, A=A, H=H, L=L, B=B, rows=a.rows, steps=a.steps, repeats=a.repeats,
               new_us=statistics.median(times["new"]), old_us=statistics.median(times["old"]),
               new_us_all=[round(t, 2) for t in times["new"]], old_us_all=[round(t, 2) for t in times["old"]],
               new_labelled_launches=sum(prof["new"].values()), old_labelled_launches=sum(prof["old"].values()),
               new_launches=prof["new"], old_launches=prof["old"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
