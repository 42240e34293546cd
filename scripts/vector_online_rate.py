"""Times the discrete lidar task and the vectorised Q-learning loop (csrc/navsim_discrete.hpp, porl_amd/env/env.py,
porl_amd/train/vector_online.py).  Three things, one JSON line each configuration:

  1. robot-steps per second of `DiscreteLidarNavSim.step` (porl_nav_dstep) with auto_reset at N in {1, 1024, 65536}
     in the lattice world, with and without a replay target, next to `LidarNavSim.step` (the continuous task, the same
     casts) measured in the same process.  Median of REPS windows of INNER back-to-back steps between two device events
     after a warm-up; at N = 1 the window is the host's launch rate, not the kernel.
  2. the whole-iteration rate of `train_vectorized` at N = 1024, S = 362, hidden [64, 64], batch 256, learn_per_step = 1:
     wall time of a call (which ends in its one read-back) after a warm-up call, transitions/s and learn steps/s.
  3. the same network trained by the route there was before: `DQNTrainer.train_online` over the single-robot `Env`,
     learning from 256 rows on, wall time around the call; the same two rates, and the ratio of 2. to 3.

Figures come from one machine; DESIGN.md quotes them."""
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
from porl_amd.env import DiscreteLidarNavSim, Env, LidarNavSim, NavWorld, random_command  # noqa: E402
from porl_amd.net.q_network import QNetwork  # noqa: E402
from porl_amd.train.dqn_trainer import DQNTrainer  # noqa: E402

REPS, INNER = 5, 20
dev = torch.device("cuda", 0)
LOGS = tempfile.mkdtemp()


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


def emit(**res):
    print(json.dumps({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


# ---- 1. the step kernel ---------------------------------------------------------------------------------------------------
world = NavWorld.lattice()
for n in (1, 1024, 65536):
    gen = torch.Generator(device=dev).manual_seed(0)
    cont = LidarNavSim(world, n, seed=1, auto_reset=True, device=dev)
    cont.reset()
    cmd = random_command(n, gen, dev)
    disc = DiscreteLidarNavSim(world, n, seed=1, auto_reset=True, device=dev)
    disc.reset()
    acts = torch.randint(0, 5, (n,), generator=gen, device=dev)
    replay = DeviceReplay(max(4 * n, 4096), disc.obs_dim, dev)
    res = {}
    for _ in range(2):                                           # the variants alternate, twice: the spread is in min / max
        for name, fn in (("continuous", lambda: cont.step(cmd)), ("discrete", lambda: disc.step(acts)),
                         ("discrete_replay", lambda: disc.step(acts, replay=replay))):
            res.setdefault(name, []).append(window_ms(fn, INNER))
    for name, runs in res.items():
        ms = statistics.median(r[0] for r in runs)
        emit(bench="nav_dstep", variant=name, n_envs=n, beams=360, step_ms=ms, step_ms_min=min(r[1] for r in runs),
             step_ms_max=max(r[2] for r in runs), robot_steps_per_s=round(n / ms * 1e3))
    assert not bool((disc.counters[:, 2] & 256).any())
    del cont, disc, replay
    torch.cuda.empty_cache()


# ---- 2. train_vectorized --------------------------------------------------------------------------------------------------
def trainer():
    torch.manual_seed(0)
    return DQNTrainer(362, 5, 0.99, device=dev, batch_size=256, log_dir=LOGS, network=lambda s, a: QNetwork(s, a, [64, 64]),
                      transition_learning_step=256)


N_VEC, STEPS = 1024, 4000
t = trainer()
sim = DiscreteLidarNavSim(world, N_VEC, seed=2, auto_reset=True, device=dev)
rep = DeviceReplay(100000, 362, dev)
kw = dict(replay=rep, learn_per_step=1, learning_starts=256, block=32, seed=0)
t.train_vectorized(sim, 40, **kw)                                # warm-up: every kernel of the loop has run
walls = []
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = t.train_vectorized(sim, STEPS, **kw)                   # ends in its read-back
    walls.append(time.perf_counter() - t0)
wall = statistics.median(walls)
vec_tr, vec_ls = N_VEC * STEPS / wall, out["learn_steps"] / wall
emit(bench="train_vectorized", n_envs=N_VEC, state=362, hidden=[64, 64], batch=256, steps=STEPS, wall_s=wall, wall_s_min=min(walls),
     wall_s_max=max(walls), transitions_per_s=round(vec_tr), learn_steps_per_s=round(vec_ls), iteration_ms=wall / STEPS * 1e3,
     can_sample=bool(t._engine.can_sample), episodes=float(out["tallies"][0]), last_loss=float(out["losses"][-1]))

# ---- 3. the single-robot route: train_online over Env ---------------------------------------------------------------------
t1 = trainer()
env = Env(5, 362, seed=2)
np.random.seed(0)
EPISODES, MAX_STEPS = 150, 200
with contextlib.redirect_stdout(io.StringIO()):
    while t1.optimizer.step_count < 50:                          # warm-up: the buffer passes the learn threshold, kernels have run
        t1.train_online(env, num_episodes=1, max_steps=MAX_STEPS)
    rows0, steps0 = len(t1.replay_buffer), t1.optimizer.step_count
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t1.train_online(env, num_episodes=EPISODES, max_steps=MAX_STEPS)
    torch.cuda.synchronize()
    wall1 = time.perf_counter() - t0
rows, learns = len(t1.replay_buffer) - rows0, t1.optimizer.step_count - steps0
emit(bench="train_online_env", n_envs=1, state=362, hidden=[64, 64], batch=256, transitions=rows, learn_steps=learns, wall_s=wall1,
     transitions_per_s=round(rows / wall1), learn_steps_per_s=round(learns / wall1))
emit(bench="ratio", transitions_per_s=vec_tr / (rows / wall1), learn_steps_per_s=vec_ls / max(learns / wall1, 1e-9),
     note="one machine, one run each")
