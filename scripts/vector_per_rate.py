"""Times prioritized replay in the vectorised loop (csrc/per_vector.hpp, porl_amd/train/vector_per.py).  One JSON line per
configuration, printed and appended to --out (default profiles/vector_per_rate.jsonl):

  1. `porl_per_fill_range` at n in {64, 1024, 65536} in a capacity-100 000 and a capacity-1 048 576 tree, next to what it
     replaces, `porl_per_update` over an arange of the same slots (three launches, an index tensor and a td tensor that
     already exist).  Median of REPS windows of INNER back-to-back calls between two device events after a warm-up; the two
     alternate, twice, and the spread is in min / max.  At small n a window measures the host's launch rate.
  2. the whole-iteration rate of `PERTrainer.train_vectorized_per` at N = 1024, S = 362, hidden [64, 64], batch 256,
     learn_per_step = 1: wall time of a call (which ends in its one read-back) after a warm-up call.
  3. `DDQNTrainer.train_vectorized`, same shapes: the uniform-replay sibling — the difference is the price of prioritisation.
  4. `PERTrainer.train_online(Env(...))`, the single-robot route this agent had in this task before.

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
from porl_amd.buffer.device_replay import DeviceReplay  # noqa: E402
from porl_amd.buffer.prioritized_replay_buffer import PrioritizedReplayBuffer  # noqa: E402
from porl_amd.env import DiscreteLidarNavSim, Env, NavWorld  # noqa: E402
from porl_amd.net.q_network import QNetwork  # noqa: E402
from porl_amd.train import online  # noqa: E402
from porl_amd.train.dqn_per_trainer import PERTrainer  # noqa: E402
from porl_amd.train.dqn_trainer import DDQNTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vector_per_rate.jsonl"))
ap.add_argument("--trace-iterations", type=int, default=0)
ap.add_argument("--skip-online", action="store_true")
args = ap.parse_args()

REPS, INNER = 7, 1000
dev = torch.device("cuda", 0)
LOGS = tempfile.mkdtemp()
world = NavWorld.lattice()
N_VEC, S, A, B, STEPS = 1024, 362, 5, 256, 4000
net = lambda s, a: QNetwork(s, a, [64, 64])  # noqa: E731


def per_trainer():
    torch.manual_seed(0)
    return PERTrainer(S, A, 0.99, device=dev, batch_size=B, log_dir=LOGS, network=net, capacity=100000)


if args.trace_iterations:
    t = per_trainer()
    sim = DiscreteLidarNavSim(world, N_VEC, seed=2, auto_reset=True, device=dev)
    out = t.train_vectorized_per(sim, args.trace_iterations, learn_per_step=1, learning_starts=B, block=32, seed=0)
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


# ---- 1. the fill against porl_per_update over the same slots ----------------------------------------------------------------
for cap in (100000, 1048576):
    buf = PrioritizedReplayBuffer(cap, state_shape=(1,), device=dev)
    buf._update(torch.arange(cap, device=dev) + (cap - 1), torch.rand(cap, dtype=torch.float64, device=dev) + 0.01)
    levels = (2 * cap - 1).bit_length() - 1
    for n in (64, 1024, 65536):
        first = 12345
        idx = torch.arange(first, first + n, device=dev) + (cap - 1)
        td = torch.full((n,), 1.0, dtype=torch.float64, device=dev)
        res = {}
        for _ in range(2):
            for name, fn in (("fill_range", lambda: buf.fill_range(first, n, 1.0)), ("per_update", lambda: buf._update(idx, td))):
                res.setdefault(name, []).append(window_ms(fn, INNER))
        ms = {k: statistics.median(r[0] for r in v) for k, v in res.items()}
        for name, runs in res.items():
            emit(bench="per_fill", variant=name, capacity=cap, n=n, levels=levels, call_us=1e3 * ms[name],
                 call_us_min=1e3 * min(r[1] for r in runs), call_us_max=1e3 * max(r[2] for r in runs))
        emit(bench="per_fill_ratio", capacity=cap, n=n, per_update_over_fill=ms["per_update"] / ms["fill_range"],
             node_write_ratio=levels * n / (2.0 * n + 4 * levels))
    del buf
    torch.cuda.empty_cache()


# ---- 2. / 3. the vectorised loops --------------------------------------------------------------------------------------------
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
tp = per_trainer()
sim = DiscreteLidarNavSim(world, N_VEC, seed=2, auto_reset=True, device=dev)
kw = dict(learn_per_step=1, learning_starts=B, block=32, seed=0)
wall, lo, hi, out = time_loop(lambda k: tp.train_vectorized_per(sim, k, **kw))
rates["per"] = (N_VEC * STEPS / wall, out["learn_steps"] / wall)
emit(bench="train_vectorized_per", n_envs=N_VEC, state=S, hidden=[64, 64], batch=B, steps=STEPS, wall_s=wall, wall_s_min=lo,
     wall_s_max=hi, transitions_per_s=round(rates["per"][0]), learn_steps_per_s=round(rates["per"][1]), iteration_ms=wall / STEPS * 1e3,
     fused=bool(tp._engine.fused), episodes=float(out["tallies"][0]), last_loss=float(out["losses"][-1]),
     total_priority=out["total_priority"])
del tp, sim
torch.cuda.empty_cache()

torch.manual_seed(0)
td_ = DDQNTrainer(S, A, 0.99, device=dev, batch_size=B, log_dir=LOGS, network=net, transition_learning_step=B)
sim = DiscreteLidarNavSim(world, N_VEC, seed=2, auto_reset=True, device=dev)
rep = DeviceReplay(100000, S, dev)
wall, lo, hi, out = time_loop(lambda k: td_.train_vectorized(sim, k, replay=rep, **kw))
rates["ddqn"] = (N_VEC * STEPS / wall, out["learn_steps"] / wall)
emit(bench="train_vectorized_ddqn", n_envs=N_VEC, state=S, hidden=[64, 64], batch=B, steps=STEPS, wall_s=wall, wall_s_min=lo,
     wall_s_max=hi, transitions_per_s=round(rates["ddqn"][0]), learn_steps_per_s=round(rates["ddqn"][1]),
     iteration_ms=wall / STEPS * 1e3, can_sample=bool(td_._engine.can_sample), last_loss=float(out["losses"][-1]))
emit(bench="price_of_prioritisation", per_over_ddqn_learn_steps=rates["per"][1] / rates["ddqn"][1],
     per_over_ddqn_transitions=rates["per"][0] / rates["ddqn"][0])
del td_, sim, rep
torch.cuda.empty_cache()

# ---- 4. the single-robot route: PERTrainer.train_online over Env ------------------------------------------------------------
if not args.skip_online:
    t1 = per_trainer()
    env = Env(A, S, seed=2)
    np.random.seed(0)
    EPISODES, MAX_STEPS = 100, 200
    with contextlib.redirect_stdout(io.StringIO()):
        while t1.optimizer.step_count < 50:                      # warm-up: the memory passes the learn threshold, kernels have run
            t1.train_online(env, num_episodes=1, max_steps=MAX_STEPS)
        steps0 = t1.optimizer.step_count
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t1.train_online(env, num_episodes=EPISODES, max_steps=MAX_STEPS)
        torch.cuda.synchronize()
        wall1 = time.perf_counter() - t0
    learns = t1.optimizer.step_count - steps0                    # one transition per learn step once the threshold is passed
    emit(bench="per_train_online_env", n_envs=1, state=S, hidden=[64, 64], batch=B, transitions=learns, learn_steps=learns,
         wall_s=wall1, transitions_per_s=round(learns / wall1), learn_steps_per_s=round(learns / wall1),
         fast_path=bool(online.fast_per_ok(t1)), note="S = 362 is wider than the one-launch step kernel: the loop on select_action / add / learn")
    emit(bench="ratio_to_train_online", transitions_per_s=rates["per"][0] / (learns / wall1),
         learn_steps_per_s=rates["per"][1] / max(learns / wall1, 1e-9), note="one machine, one run each")
