"""Times the navigation simulator (csrc/navsim.hpp, porl_amd/env): steps per second of `LidarNavSim.step` with
auto_reset at N in {1, 256, 4096, 65536} robots, in the lattice world (20 primitives) and in a 512-primitive world (the
lattice plus 492 thin posts on the lattice lines, outside the spawn interiors).

Each figure is the median of REPS = 5 windows of INNER = 20 back-to-back steps between two device events, after a
warm-up (the convention of DESIGN.md §4f).  A window covers whatever the stream did between the events, so at small N it
is the host's launch rate (the wrapper's allocations and one launch), not the kernel; from N = 4096 on the device is the
slower side and step_ms is the kernel's time, the figure to compare with arithmetic.  `pairs_per_s` = robots x beams x primitives per
second.  For context only: the numpy restatement's rate (tests/helpers/navsim_cases.py, N = 256) on this host's CPU, and
the wall time of `evaluate_policy_batched` for 1 024 episodes of 500 steps of an H = 256 SORL policy.
One JSON line per configuration; DESIGN.md §4l quotes them."""
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from porl_amd.env import LidarNavSim, NavWorld, random_command  # noqa: E402

REPS, INNER = 5, 20
dev = torch.device("cuda", 0)


def dense_world():
    base = NavWorld.lattice()
    ox, oy = base.origin
    posts = []
    k = 0
    while len(posts) < 492:
        line, pos = 1 + k % 4, (k // 8 + 0.5) * 5.0 / 62
        posts.append([ox + line, oy + pos, 0.02] if (k // 4) % 2 == 0 else [ox + pos, oy + line, 0.02])
        k += 1
    cir = torch.cat([base.circles, torch.tensor(posts, dtype=torch.float32)])
    return NavWorld(base.segments, cir, origin=base.origin)


def window_ms(fn, inner):
    for _ in range(inner):
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
        times.append(e0.elapsed_time(e1) / inner)
    return statistics.median(times)


def emit(**res):
    print(json.dumps({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


for name, world in (("lattice", NavWorld.lattice()), ("dense512", dense_world())):
    prims = world.segments.shape[0] + world.circles.shape[0]
    for n in (1, 256, 4096, 65536):
        sim = LidarNavSim(world, n, seed=1, auto_reset=True, device=dev)
        sim.reset()
        gen = torch.Generator(device=dev).manual_seed(0)
        actions = random_command(n, gen, dev)
        ms = window_ms(lambda: sim.step(actions), INNER)
        assert not bool((sim.counters[:, 2] & 256).any())
        emit(bench="nav_step", world=name, primitives=prims, n_envs=n, beams=360, step_ms=ms,
             robot_steps_per_s=round(n / ms * 1e3), pairs_per_s=n * 360 * prims / ms * 1e3,
             episodes_seen=int(sim.counters[:, 1].sum()) - n)
        del sim
        torch.cuda.empty_cache()

# context: the numpy restatement on this host
from helpers import navsim_cases as NC  # noqa: E402
o = NC.Sim(NC.lattice(), 256, seed=1, auto_reset=True)
o.reset()
a = ((np.random.default_rng(0).random((256, 2)) * 2 + [0, -1]) * [0.075, 1.5]).astype(np.float32)
t0 = time.perf_counter()
for _ in range(5):
    o.step(a)
dt = (time.perf_counter() - t0) / 5
emit(bench="numpy_restatement", world="lattice", n_envs=256, step_ms=dt * 1e3, robot_steps_per_s=round(256 / dt))

# evaluate_policy_batched: 1 024 episodes of an H = 256 SORL policy, one round of 1 024 robots
from porl_amd.agent.sorl import SORL  # noqa: E402
from porl_amd.evaluate import evaluate_policy_batched, sorl_act  # noqa: E402
args = SimpleNamespace(state_size=362, hidden_dim=256, n_hidden=2, layer_norm=False, action_size=2, max_batch=1024)
agent = SORL(args, 1000, 0.9, 10.0, device=dev)
sim = LidarNavSim(NavWorld.lattice(), 1024, seed=2, device=dev)
act = sorl_act(agent)
evaluate_policy_batched(act, sim, 1024, 20)                               # warm-up
torch.cuda.synchronize()
t0 = time.perf_counter()
triple = evaluate_policy_batched(act, sim, 1024, 500)
wall = time.perf_counter() - t0
emit(bench="evaluate_policy_batched", episodes=1024, episode_step=500, hidden=256, wall_s=wall,
     robot_steps_per_s=round(1024 * 500 / wall), mean_steps=triple[0], mean_score=triple[1], success=triple[2])
