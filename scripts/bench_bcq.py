#!/usr/bin/env python3
"""Updates per second of discrete BCQ's two hot loops, the forms of the parent tree against the one-call forms:

  learn     bcq_learn (numpy index draw + H2D copy, five gathers, per-layer behaviour forward, porl_softmax_mask, step
            kernel, loss read back)  against  bcq_learn_device_sampled (mask kernel + step kernel + reduce/Adam from one
            native call, rows drawn in the kernels)
  pretrain  bcq_behavior_pretrain (index draw + copy, five gathers, step kernel, loss read back per epoch)  against
            bcq_pretrain_device_sampled (step kernel + reduce/Adam per epoch, one readback at the end)

S = 60, A = 10, default networks, a full 100 000-row buffer, batch 64 and 4096.  Each figure is the median of `--runs`
timed windows of `--steps` updates after a warm-up window, every window closed by a device synchronise; the learn forms
are timed with the loss read back every step (the default) and with agent.async_losses.  The two sides of a pair
alternate inside one process.  Prints one JSON line.

    python scripts/bench_bcq.py [--steps 300] [--runs 5] [--batches 64,4096]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from porl_amd.policy import bcq  # noqa: E402
from porl_amd.train.bcq_trainer import BCQTrainer  # noqa: E402

S, A, ROWS = 60, 10, 100_000


def trainer(B, steps):
    torch.manual_seed(0)
    t = BCQTrainer(S, A, 0.99, device="cuda", batch_size=B, max_batch=max(B, 4096), num_epochs=steps, threshold=0.1)
    rb = t.replay_buffer
    rng = np.random.default_rng(1)
    rb.states[:] = rng.standard_normal((ROWS, S), dtype=np.float32)
    rb.next_states[:] = rng.standard_normal((ROWS, S), dtype=np.float32)
    rb.actions[:] = rng.integers(A, size=ROWS)
    rb.rewards[:] = rng.standard_normal(ROWS, dtype=np.float32)
    rb.dones[:] = (rng.random(ROWS) < 0.05).astype(np.float32)
    rb.size, rb.position = ROWS, 0
    rb._sync_mirror()
    return t


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batches", default="64,4096")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bcq.py measures on a HIP device; none is visible")
    out = {"state_dim": S, "n_actions": A, "rows": ROWS, "steps": args.steps, "runs": args.runs, "results": {}}
    for B in (int(b) for b in args.batches.split(",")):
        t = trainer(B, args.steps)
        np.random.seed(0)

        def loop(fn):
            return lambda n: [fn(t) for _ in range(n)]

        def asynchronous(fn):
            def run(n):
                t.async_losses = True
                try:
                    for _ in range(n):
                        fn(t)
                finally:
                    t.async_losses = False
            return run
        forms = {
            "learn_parent": loop(bcq.bcq_learn),
            "learn_device_sampled": loop(bcq.bcq_learn_device_sampled),
            "learn_parent_async": asynchronous(bcq.bcq_learn),
            "learn_device_sampled_async": asynchronous(bcq.bcq_learn_device_sampled),
            "pretrain_parent": lambda n: bcq.bcq_behavior_pretrain(t),                 # num_epochs == steps
            "pretrain_device_sampled": lambda n: bcq.bcq_pretrain_device_sampled(t),
        }
        rates = {k: [] for k in forms}
        for k, fn in forms.items():                                                   # warm-up: every form, every shape
            window(fn, args.steps)
        for _ in range(args.runs):                                                    # alternate the forms
            for k, fn in forms.items():
                rates[k].append(window(fn, args.steps))
        out["results"][str(B)] = {k: {"median_updates_per_s": round(statistics.median(v), 1),
                                      "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in rates.items()}
        out["results"][str(B)]["one_launch"] = dict(q=bool(t._engine.fused), behaviour=bool(t._behavior_engine.fused),
                                                    in_kernel_sampling=bool(t._engine.can_sample))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
