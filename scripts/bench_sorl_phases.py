"""Two-phase SORL training, phase two: steps/s of `SORL.policy_update_from_replay` (policy-only step, value nets frozen)
beside `SORL.update_from_replay` (joint step, non-pipelined form), and the launch count of one policy-only step from the
in-process profiler.  Stand-alone:  python scripts/bench_sorl_phases.py [--steps 300] [--runs 5] [--joint-only]

Each shape: warm-up, then `--runs` timed windows per method, the two methods alternating; the median window is
reported, with the lowest and highest beside it.  A window ends in a device synchronisation."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from types import SimpleNamespace
from porl_amd import engine as E
from porl_amd.agent.sorl import SORL
from porl_amd.buffer.replay_buffer import PackedReplay
from porl_amd.util.synth import make_rows

SHAPES = [("headline", 60, 1024, 1024), ("config5-heads", 256, 512, 512)]       # name, S (feature width), H, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--joint-only", action="store_true", help="time update_from_replay only (a tree without the policy-only step)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    for name, S, H, B in SHAPES:
        torch.manual_seed(0)
        agent = SORL(SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=2, layer_norm=False, action_size=2, max_batch=B),
                     10 ** 6, 0.9, 1.0, device=dev)
        agent.async_losses = True            # no host read-back per step ...
        agent.pipeline = False               # ... and the joint step in its one-stream form (porl_iql_step)
        rp = PackedReplay(make_rows(100_000, S, 2, seed=1), S, 2, dev, seed=2)
        methods = {"update_from_replay": agent.update_from_replay}
        if not a.joint_only:
            methods["policy_update_from_replay"] = agent.policy_update_from_replay
        for fn in methods.values():
            for _ in range(a.warmup):
                fn(rp, B)
        torch.cuda.synchronize()
        rates = {m: [] for m in methods}
        for _ in range(a.runs):
            for m, fn in methods.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn(rp, B)
                torch.cuda.synchronize()
                rates[m].append(a.steps / (time.perf_counter() - t0))
        out = dict(shape=name, S=S, H=H, B=B, steps=a.steps, runs=a.runs)
        for m, v in rates.items():
            out[m] = dict(median_steps_per_s=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))
        if not a.joint_only:
            out["ratio"] = round(out["policy_update_from_replay"]["median_steps_per_s"] / out["update_from_replay"]["median_steps_per_s"], 3)
            n = 20
            for m, fn in methods.items():
                E.prof_enable(True)
                for _ in range(n):
                    fn(rp, B)
                prof = [p for p in E.prof_read() if p["launches"]]
                E.prof_enable(False)
                out[m]["launches_per_step"] = sum(p["launches"] for p in prof) / n
                out[m]["kernel_us_per_step"] = round(sum(p["total_ms"] for p in prof) * 1e3 / n, 1)
                if m == "policy_update_from_replay":
                    out["policy_only_kernels_us"] = {p["name"]: round(p["total_ms"] * 1e3 / p["launches"], 1)
                                                     for p in sorted(prof, key=lambda p: p["name"])}
        print(json.dumps(out), flush=True)
        del agent, rp


if __name__ == "__main__":
    main()
