"""Times C51 and QR-DQN in the vectorised loop (csrc/dist_act.hpp, porl_amd/train/vector_dist.py).  One JSON line per
configuration, printed and appended to --out (default profiles/vector_dist_rate.jsonl):

  1. `engine.dist_select` at n in {1024, 65536}, A = 5, n_sub = 51, both heads, next to the route the tree had to the same
     actions before: a torch expression over the (n, 255) outputs (the quantile mean, or the softmax expectation over the
     support) followed by `engine.qnet_select`.  Median of REPS windows of INNER back-to-back calls between two device
     events after a warm-up; the two alternate, twice, and the spread is in min / max.  At n = 1024 a window measures the
     host's launch rate: the torch route is 2 (QR) or 4 (C51) calls and an allocation per torch operator, the kernel one and none.
  2. the whole-iteration rate of `C51Trainer` / `QRDQNTrainer.train_vectorized_dist` at N = 1024, S = 362, hidden
     [128, 128], batch 256, learn_per_step = 1: wall time of a call (which ends in its one read-back) after a warm-up call.
  3. `DDQNTrainer.train_vectorized`, same shapes: the plain-Q sibling in the same process.
  4. `train_online(Env(5, 362))` of the same two trainers, the single-robot route they had in this task before.

`--trace-iterations K --kind c51|qr` runs only K iterations of 2. after construction (for a kernel trace: calls / K =
launches per iteration).  Figures come from one machine; DESIGN.md quotes them."""
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
from porl_amd import _native as N  # noqa: E402
from porl_amd import engine as E  # noqa: E402
from porl_amd.buffer.device_replay import DeviceReplay  # noqa: E402
from porl_amd.env import DiscreteLidarNavSim, Env, NavWorld  # noqa: E402
from porl_amd.net.q_network import QNetwork  # noqa: E402
from porl_amd.train.c51_trainer import C51Trainer  # noqa: E402
from porl_amd.train.dqn_trainer import DDQNTrainer  # noqa: E402
from porl_amd.train.qr_dqn_trainer import QRDQNTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vector_dist_rate.jsonl"))
ap.add_argument("--trace-iterations", type=int, default=0)
ap.add_argument("--kind", choices=("c51", "qr"), default="c51")
ap.add_argument("--skip-online", action="store_true")
args = ap.parse_args()

REPS, INNER = 7, 1000
dev = torch.device("cuda", 0)
LOGS = tempfile.mkdtemp()
world = NavWorld.lattice()
N_VEC, S, A, NS, B, STEPS, HIDDEN = 1024, 362, 5, 51, 256, 4000, [128, 128]


def dist_trainer(kind):
    torch.manual_seed(0)
    if kind == "c51":
        return C51Trainer(S, A, 0.99, device=dev, batch_size=B, log_dir=LOGS, atom_size=NS, network_hidden_sizes=HIDDEN)
    return QRDQNTrainer(S, A, 0.99, device=dev, batch_size=B, log_dir=LOGS, num_quantiles=NS, network_hidden_sizes=HIDDEN,
                        transition_learning_step=B)


if args.trace_iterations:
    t = dist_trainer(args.kind)
    sim = DiscreteLidarNavSim(world, N_VEC, seed=2, auto_reset=True, device=dev)
    out = t.train_vectorized_dist(sim, args.trace_iterations, learn_per_step=1, learning_starts=B, block=32, seed=0)
    print(json.dumps(dict(bench="trace", kind=args.kind, iterations=args.trace_iterations, learn_steps=out["learn_steps"])), flush=True)
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


# ---- 1. the select kernel against the torch expression + qnet_select ------------------------------------------------------
support = torch.linspace(-10.0, 10.0, NS, device=dev)
heads = dict(qr=N.DistHead(0, A, NS, 1.0, 0.0, 0.0, None), c51=N.DistHead(1, A, NS, 0.0, -10.0, 10.0, support.data_ptr()))
for n in (1024, 65536):
    z = torch.randn(n, A * NS, device=dev)
    q, out = torch.empty(n, A, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    inner = INNER if n == 1024 else 200
    for kind, head in heads.items():
        def kernel():
            E.dist_select(z, head, 0.1, 3, 7, q=q, out=out)

        def torch_route():
            v = z.view(n, A, NS)
            vals = v.mean(2) if kind == "qr" else (torch.softmax(v, 2) * support).sum(2)
            E.qnet_select(vals, 0.1, 3, 7, out=out)

        kernel()
        mine = out.clone()
        torch_route()
        agree = float((mine == out).float().mean())              # (summation orders differ: near-ties may not)
        res = {}
        for _ in range(2):
            for name, fn in (("dist_select", kernel), ("torch_then_qnet_select", torch_route)):
                res.setdefault(name, []).append(window_ms(fn, inner))
        ms = {k: statistics.median(r[0] for r in v) for k, v in res.items()}
        for name, runs in res.items():
            emit(bench="dist_select", head=kind, variant=name, n=n, n_actions=A, n_sub=NS, call_us=1e3 * ms[name],
                 call_us_min=1e3 * min(r[1] for r in runs), call_us_max=1e3 * max(r[2] for r in runs))
        emit(bench="dist_select_ratio", head=kind, n=n, torch_over_kernel=ms["torch_then_qnet_select"] / ms["dist_select"],
             same_actions=agree, input_gb_per_s=n * A * NS * 4 / (ms["dist_select"] * 1e-3) / 1e9)
    del z, q, out
    torch.cuda.empty_cache()


# ---- 2. / 3. the vectorised loops ------------------------------------------------------------------------------------------
def time_loop(call):
    call(40)                                                     # warm-up: every kernel of the loop has run
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call(STEPS)                                        # ends in its read-back
        walls.append(time.perf_counter() - t0)
    return statistics.median(walls), min(walls), max(walls), out


rates = {}
kw = dict(learn_per_step=1, learning_starts=B, block=32, seed=0)
for kind in ("c51", "qr"):
    t = dist_trainer(kind)
    sim = DiscreteLidarNavSim(world, N_VEC, seed=2, auto_reset=True, device=dev)
    rep = DeviceReplay(100000, S, dev)
    wall, lo, hi, out = time_loop(lambda k: t.train_vectorized_dist(sim, k, replay=rep, **kw))
    rates[kind] = (N_VEC * STEPS / wall, out["learn_steps"] / wall)
    emit(bench="train_vectorized_dist", kind=kind, n_envs=N_VEC, state=S, hidden=HIDDEN, n_sub=NS, batch=B, steps=STEPS, wall_s=wall,
         wall_s_min=lo, wall_s_max=hi, transitions_per_s=round(rates[kind][0]), learn_steps_per_s=round(rates[kind][1]),
         iteration_ms=wall / STEPS * 1e3, episodes=float(out["tallies"][0]), last_loss=float(out["losses"][-1]))
    del t, sim, rep
    torch.cuda.empty_cache()

torch.manual_seed(0)
td_ = DDQNTrainer(S, A, 0.99, device=dev, batch_size=B, log_dir=LOGS, network=lambda s, a: QNetwork(s, a, HIDDEN),
                  transition_learning_step=B)
sim = DiscreteLidarNavSim(world, N_VEC, seed=2, auto_reset=True, device=dev)
rep = DeviceReplay(100000, S, dev)
wall, lo, hi, out = time_loop(lambda k: td_.train_vectorized(sim, k, replay=rep, **kw))
rates["ddqn"] = (N_VEC * STEPS / wall, out["learn_steps"] / wall)
emit(bench="train_vectorized_ddqn", n_envs=N_VEC, state=S, hidden=HIDDEN, batch=B, steps=STEPS, wall_s=wall, wall_s_min=lo,
     wall_s_max=hi, transitions_per_s=round(rates["ddqn"][0]), learn_steps_per_s=round(rates["ddqn"][1]),
     iteration_ms=wall / STEPS * 1e3, fused=bool(td_._engine.fused), last_loss=float(out["losses"][-1]))
for kind in ("c51", "qr"):
    emit(bench="dist_over_ddqn", kind=kind, learn_steps=rates[kind][1] / rates["ddqn"][1], transitions=rates[kind][0] / rates["ddqn"][0])
del td_, sim, rep
torch.cuda.empty_cache()

# ---- 4. the single-robot route: train_online over Env -----------------------------------------------------------------------
if not args.skip_online:
    for kind in ("c51", "qr"):
        t1 = dist_trainer(kind)
        env = Env(A, S, seed=2)
        np.random.seed(0)
        EPISODES, MAX_STEPS = 100, 200
        with contextlib.redirect_stdout(io.StringIO()):
            while t1.optimizer.step_count < 50:                  # warm-up: the buffer passes the learn threshold, kernels have run
                t1.train_online(env, num_episodes=1, max_steps=MAX_STEPS)
            steps0 = t1.optimizer.step_count
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t1.train_online(env, num_episodes=EPISODES, max_steps=MAX_STEPS)
            torch.cuda.synchronize()
            wall1 = time.perf_counter() - t0
        learns = t1.optimizer.step_count - steps0                # one transition per learn step once the threshold is passed
        emit(bench="dist_train_online_env", kind=kind, n_envs=1, state=S, hidden=HIDDEN, n_sub=NS, batch=B, transitions=learns,
             learn_steps=learns, wall_s=wall1, transitions_per_s=round(learns / wall1), learn_steps_per_s=round(learns / wall1))
        emit(bench="ratio_to_train_online", kind=kind, transitions_per_s=rates[kind][0] / (learns / wall1),
             learn_steps_per_s=rates[kind][1] / max(learns / wall1, 1e-9), note="one machine, one run each")
        del t1, env
