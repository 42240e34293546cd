"""Times IQN in the vectorised loop (csrc/iqn_vector.hpp, porl_amd/train/vector_iqn.py).  One JSON line per configuration,
printed and appended to --out (default profiles/vector_iqn_rate.jsonl):

  1. `engine.iqn_select_rows` at n in {1024, 65536}, K = 32 fractions, A = 5 (ld = 8), next to the route the tree had to
     the same actions before: `z.view(n, K, ld)[..., :A].mean(1)` followed by `engine.qnet_select`.  Median of REPS
     windows of INNER back-to-back calls between two device events after a warm-up; the two alternate, twice, and the spread
     is in min / max.  At n = 1024 a window measures the host's launch rate: the torch route is two calls and an allocation,
     the kernel one and none.
  2. the whole-iteration rate of `IQNTrainer.train_vectorized_iqn` at N = 1024, S = 362, the trainer's default network
     (hidden 512, embedding 64, 32 / 8 / 8 fractions), batch 256, learn_per_step = 1: wall time of a call (which ends in its
     one read-back) after a warm-up call; three calls.
  3. `IQNTrainer.train_online(Env(5, 362))` in the same process, the single-robot route the trainer had in this task before.

`--trace-iterations K` runs only K iterations of 2. after construction (for a kernel trace: calls / K = launches per
iteration).  Figures come from one machine; DESIGN.md quotes them."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from porl_amd import engine as E  # noqa: E402
from porl_amd.buffer.device_replay import DeviceReplay  # noqa: E402
from porl_amd.env import DiscreteLidarNavSim, Env, NavWorld  # noqa: E402
from porl_amd.train.iqn_trainer import IQNTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vector_iqn_rate.jsonl"))
ap.add_argument("--trace-iterations", type=int, default=0)
ap.add_argument("--skip-online", action="store_true")
args = ap.parse_args()

REPS, INNER = 7, 1000
dev = torch.device("cuda", 0)
LOGS = tempfile.mkdtemp()
world = NavWorld.lattice()
N_VEC, S, A, B, STEPS = 1024, 362, 5, 256, 1000


def iqn_trainer():
    torch.manual_seed(0)
    return IQNTrainer(S, A, 0.99, device=dev, batch_size=B, log_dir=LOGS, transition_learning_step=B)


kw = dict(learn_per_step=1, learning_starts=B, block=32, seed=0)
if args.trace_iterations:
    t = iqn_trainer()
    sim = DiscreteLidarNavSim(world, N_VEC, seed=2, auto_reset=True, device=dev)
    out = t.train_vectorized_iqn(sim, args.trace_iterations, **kw)
    print(json.dumps(dict(bench="trace", iterations=args.trace_iterations, learn_steps=out["learn_steps"])), flush=True)
    sys.exit(0)

sink = open(args.out, "a")


def emit(**res):
    line = json.dumps({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in res.items()})
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


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
    return statistics.median(times), min(times), max(times)


# ---- 1. the rows head against the torch mean + qnet_select -----------------------------------------------------------------
K, LD = 32, 8
for n in (1024, 65536):
    z = torch.randn(n * K, LD, device=dev)
    q, out = torch.empty(n, A, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    inner = INNER if n == 1024 else 200

    def kernel():
        E.iqn_select_rows(z[:, :A], K, 0.1, 3, 7, q=q, out=out)

    def torch_route():
        E.qnet_select(z.view(n, K, LD)[..., :A].mean(1), 0.1, 3, 7, out=out)

    kernel()
    mine = out.clone()
    torch_route()
    agree = float((mine == out).float().mean())                  # (summation orders differ: near-ties may not)
    res = {}
    for _ in range(2):
        for name, fn in (("iqn_select_rows", kernel), ("torch_mean_then_qnet_select", torch_route)):
            res.setdefault(name, []).append(window_ms(fn, inner))
    ms = {k: statistics.median(r[0] for r in v) for k, v in res.items()}
    for name, runs in res.items():
        emit(bench="iqn_select_rows", variant=name, n=n, n_tau=K, n_actions=A, ld=LD, call_us=1e3 * ms[name],
             call_us_min=1e3 * min(r[1] for r in runs), call_us_max=1e3 * max(r[2] for r in runs))
    emit(bench="iqn_select_rows_ratio", n=n, torch_over_kernel=ms["torch_mean_then_qnet_select"] / ms["iqn_select_rows"],
         same_actions=agree, input_gb_per_s=n * K * LD * 4 / (ms["iqn_select_rows"] * 1e-3) / 1e9)
    del z, q, out
    torch.cuda.empty_cache()


# ---- 2. the vectorised loop -------------------------------------------------------------------------------------------------
t = iqn_trainer()
sim = DiscreteLidarNavSim(world, N_VEC, seed=2, auto_reset=True, device=dev)
rep = DeviceReplay(100000, S, dev)
t.train_vectorized_iqn(sim, 40, replay=rep, **kw)               # warm-up: every kernel of the loop has run
walls = []
for call in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = t.train_vectorized_iqn(sim, STEPS, replay=rep, **kw)  # ends in its read-back
    wall = time.perf_counter() - t0
    emit(bench="train_vectorized_iqn", call=call, n_envs=N_VEC, state=S, hidden=512, embedding=64, n_policy=t.num_quantiles_n_policy,
         n_prime=t.num_quantiles_n_prime_loss, n_double_prime=t.num_quantiles_n_double_prime_loss, batch=B, steps=STEPS,
         wall_s=wall, transitions_per_s=round(N_VEC * STEPS / wall), learn_steps_per_s=round(out["learn_steps"] / wall),
         iteration_ms=wall / STEPS * 1e3, episodes=float(out["tallies"][0]), last_loss=float(out["losses"][-1]))
    walls.append(wall)
rate = (N_VEC * STEPS / statistics.median(walls), STEPS / statistics.median(walls))      # every timed iteration learns
del t, sim, rep
torch.cuda.empty_cache()

# ---- 3. the single-robot route: train_online over Env -----------------------------------------------------------------------
if not args.skip_online:
    t1 = iqn_trainer()
    env = Env(A, S, seed=2)
    np.random.seed(0)
    EPISODES, MAX_STEPS = 20, 200
    with contextlib.redirect_stdout(io.StringIO()):
        while t1.optimizer.step_count < 50:                      # warm-up: the buffer passes the learn threshold, kernels have run
            t1.train_online(env, num_episodes=1, max_steps=MAX_STEPS)
        steps0 = t1.optimizer.step_count
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t1.train_online(env, num_episodes=EPISODES, max_steps=MAX_STEPS)
        torch.cuda.synchronize()
        wall1 = time.perf_counter() - t0
    learns = t1.optimizer.step_count - steps0                    # one transition per learn step once the threshold is passed
    emit(bench="iqn_train_online_env", n_envs=1, state=S, batch=B, transitions=learns, learn_steps=learns, wall_s=wall1,
         transitions_per_s=round(learns / wall1), learn_steps_per_s=round(learns / wall1))
    emit(bench="ratio_to_train_online", transitions_per_s=rate[0] / (learns / wall1),
         learn_steps_per_s=rate[1] / max(learns / wall1, 1e-9), note="one machine; the median of the three vectorised calls")
