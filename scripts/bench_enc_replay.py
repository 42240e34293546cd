"""SORL + FasterNet fed from a device-resident PackedReplay, two ways on the same commit:

  rows    : agent.update_from_replay(replay, B)              index draw, encoder on the store's rows in place, indexed load
  tensors : replay.sample(B) + replay.split + agent.update   index draw, gather, two in-place clamps, pack

Both loops do the same arithmetic on the same draws (tests/test_enc_replay_gpu.py pins them bit for bit), so the
difference is one gather of B x (2S + 2 + A) floats, two clamp launches and the Python slicing per update.
B = 512 on a store of 20 000 rows, bf16 84x84 and fp32 360x256.  Timed with device events after a warm-up, the two loops
alternating, five runs each; the medians are reported.  One JSON line per configuration.

    python scripts/bench_enc_replay.py [--runs 5] [--batch 512] [--rows 20000]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [  # name, angle_bins, dist_bins, compute_dtype, steps per timed run, warm-up steps
    ("bf16_84x84", 84, 84, "bf16", 200, 20),
    ("fp32_360x256", 360, 256, "fp32", 12, 3),
]


def lidar_rows(n_rows, n_ang, act_dim, seed):
    """porl_amd.util.synth rows (rewards, terminals, actions, layout) with lidar-like states in both state blocks, as
    bench.py's sorl_enc workload draws them: beams in (0.15, 3.9), goal in (-3, 3)^2."""
    from porl_amd.util.synth import make_rows
    S = n_ang + 2
    rows = make_rows(n_rows, S, act_dim, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for off in (0, S + 1):
        rows[:, off:off + n_ang] = rng.uniform(0.15, 3.9, size=(n_rows, n_ang))
        rows[:, off + n_ang:off + S] = rng.uniform(-3, 3, size=(n_rows, 2))
    return rows


def build(n_ang, n_dist, dtype, B, dev):
    from porl_amd.agent.fasternet import FasterNet
    from porl_amd.agent.sorl import SORL
    torch.manual_seed(0)
    backbone = FasterNet(3, 256, max_batch=B, angle_bins=n_ang, dist_bins=n_dist, compute_dtype=dtype)
    args = SimpleNamespace(state_size=n_ang + 2, feature_dim=256, hidden_dim=512, n_hidden=2, layer_norm=False,
                           action_size=2, max_batch=B)
    agent = SORL(args, max_steps=100000, tau=0.9, alpha=3.0, device=dev, backbone=backbone)
    agent.async_losses = True
    return agent


def timed(step, steps, agent, dev):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(steps):
        step()
    agent.flush()                                   # the last policy phase runs on the side stream
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps              # ms per update


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rows", type=int, default=20000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_enc_replay needs a HIP device")
    from porl_amd.buffer.replay_buffer import PackedReplay
    dev = torch.device("cuda", torch.cuda.current_device())
    B = a.batch
    for name, n_ang, n_dist, dtype, steps, warm in CONFIGS:
        S, A = n_ang + 2, 2
        rows = lidar_rows(a.rows, n_ang, A, seed=0)
        agents = {k: build(n_ang, n_dist, dtype, B, dev) for k in ("rows", "tensors")}
        replays = {k: PackedReplay(rows, S, A, dev, seed=1) for k in agents}

        def step_rows(ag=agents["rows"], rp=replays["rows"]):
            ag.update_from_replay(rp, B)

        def step_tensors(ag=agents["tensors"], rp=replays["tensors"]):
            s, r, s2, d, act = rp.split(rp.sample(B))
            ag.update(s, act, r, s2, d)

        loops = {"rows": step_rows, "tensors": step_tensors}
        for k, f in loops.items():
            for _ in range(warm):
                f()
            agents[k].flush()
        ms = {k: [] for k in loops}
        for _ in range(a.runs):                     # alternate the two loops: drift hits both alike
            for k, f in loops.items():
                ms[k].append(timed(f, steps, agents[k], dev))
        losses = {k: agents[k]._engine.stats[:2].cpu().tolist() for k in loops}
        if not all(np.isfinite(v).all() for v in losses.values()):
            raise RuntimeError("non-finite loss")
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({
            "config": name, "batch": B, "store_rows": a.rows, "steps_per_run": steps, "runs": a.runs,
            "ms_per_update_median": {k: round(v, 4) for k, v in med.items()},
            "ms_per_update_runs": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "rows_over_tensors": round(med["rows"] / med["tensors"], 4),
        }), flush=True)


if __name__ == "__main__":
    main()
