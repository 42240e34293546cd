"""Times the A* expert of the lidar navigation task (csrc/expert.hpp, porl_amd/env/expert.py) and counts what it reaches.
One JSON line per configuration, printed and appended to --out (default profiles/expert_rate.jsonl):

  1. one `expert()` call at N in {1, 1024, 65536} lattice robots (the largest N the cache limit allows, if it refuses
     65536), two ways — every field fresh (each block of the field kernel returns at once) and every tag cleared before the
     call (every robot relaxes) — next to `sim.step` at the same N in the same process.  Median of REPS windows of INNER
     back-to-back calls between two device events after a warm-up.
  2. goals, hits and timeouts of 1 024 lattice episodes for inflate in {0.15, 0.18, 0.22} and lookahead in {2, 3, 4}, for
     the continuous task (evaluate_policy_batched's loop) and the discrete one (the expert's scores through
     engine.qnet_select at epsilon 0), both at the simulators' own step limit of 500.

Figures come from one machine; DESIGN.md quotes them."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
from porl_amd import engine as E  # noqa: E402
from porl_amd.env import AStarExpert, DiscreteLidarNavSim, LidarNavSim, NavWorld, PlanGrid  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "expert_rate.jsonl"))
ap.add_argument("--skip-rollouts", action="store_true")
args = ap.parse_args()

REPS = 5
dev = torch.device("cuda", 0)
world = NavWorld.lattice().to(dev)
sink = open(args.out, "a")


def emit(**res):
    line = json.dumps({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in res.items()})
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


def window_us(fn, inner):
    for _ in range(max(inner // 10, 3)):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        times.append(1e3 * e0.elapsed_time(e1) / inner)
    return statistics.median(times), min(times), max(times)


# ---- 1. one act call, beside one simulator step ----------------------------------------------------------------------------
for n in (1, 1024, 65536):
    sim = LidarNavSim(world, n, seed=3, auto_reset=True)
    sim.reset()
    try:
        ex = AStarExpert(sim)
    except ValueError as e:
        emit(bench="expert_act", n=n, refused=str(e))
        continue
    out = torch.empty(n, 2, dtype=torch.float32, device=dev)
    ex(out=out)
    inner = 200 if n <= 1024 else 10

    def fresh():
        ex(out=out)

    def cleared():
        ex.tags.zero_()
        ex(out=out)

    def zero_only():
        ex.tags.zero_()

    cmd = out.clone()

    def step():
        sim.step(cmd)

    res = dict(fresh=window_us(fresh, inner), cleared=window_us(cleared, inner), tags_zero=window_us(zero_only, inner))
    res["sim_step"] = window_us(step, inner)
    for name, (med, lo, hi) in res.items():
        emit(bench="expert_act", variant=name, n=n, call_us=med, call_us_min=lo, call_us_max=hi)
    emit(bench="expert_act_ratio", n=n, fresh_over_step=res["fresh"][0] / res["sim_step"][0],
         cleared_over_step=(res["cleared"][0] - res["tags_zero"][0]) / res["sim_step"][0],
         cache_bytes=ex.fields.numel() * 4)
    del sim, ex, out, cmd
    torch.cuda.empty_cache()

# ---- 2. what the expert reaches ------------------------------------------------------------------------------------------------
if not args.skip_rollouts:
    EPISODES, STEPS = 1024, 500
    for inflate in (0.15, 0.18, 0.22):
        grid = PlanGrid(world, inflate=inflate)
        for lookahead in (2, 3, 4):
            sim = LidarNavSim(world, EPISODES, seed=11)
            ex = AStarExpert(sim, grid=grid, lookahead=lookahead)
            sim.reset()
            for _ in range(STEPS):
                sim.step(ex())
            status = (sim.counters[:, 2] & 0xff).cpu()
            emit(bench="expert_rollout", task="continuous", inflate=inflate, lookahead=lookahead, episodes=EPISODES,
                 goals=int((status == 2).sum()), hits=int((status == 1).sum()), timeouts=int((status == 3).sum()))
            dsim = DiscreteLidarNavSim(world, EPISODES, seed=11)
            dex = AStarExpert(dsim, grid=grid, lookahead=lookahead)
            dsim.reset()
            table = torch.empty(EPISODES, dsim.n_actions, dtype=torch.float32, device=dev)
            actions = torch.empty(EPISODES, dtype=torch.int64, device=dev)
            for t in range(STEPS):
                E.qnet_select(dex(out=table), 0.0, 11, t, out=actions)
                dsim.step(actions)
            episodes, _, goals, hits = dsim.tallies.sum(0).cpu().tolist()
            emit(bench="expert_rollout", task="discrete", inflate=inflate, lookahead=lookahead, episodes=int(episodes),
                 goals=int(goals), hits=int(hits), timeouts=int(episodes - goals - hits))
