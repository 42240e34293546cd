"""Times the episode passes (csrc/episodes.hpp) on 1 M packed rows of S=60 resident in HBM — the episode table without
and with a cap of 500, the episode returns + range, and 1 000 hindsight-pair batches of B=1024 (draw + gather) — and
the numpy restatement of the reference's functions (tests/helpers/episode_cases.py) on the same rows on the host.
One JSON line; DESIGN.md §4h quotes it."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from helpers import episode_cases as EC  # noqa: E402
from porl_amd.buffer.replay_buffer import PackedReplay  # noqa: E402
from porl_amd.dataloader import episodes as EP  # noqa: E402

S, A, N, B, CAP, BATCHES = 60, 2, 1_000_000, 1024, 500, 1000
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
rows = rng.standard_normal((N, 2 * S + 2 + A)).astype(np.float32)
rows[:, S] *= 1e3
rows[:, 2 * S + 1] = (rng.random(N) < 1 / 700).astype(np.float32)
replay = PackedReplay(rows, S, A, dev, seed=0)
rew, done = replay.rows[:, S], replay.rows[:, 2 * S + 1]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


res = {"rows": N, "obs_dim": S, "batch": B, "cap": CAP}
res["table_ms"], (starts, ends, _) = timed(lambda: EP.episode_table(done, 0), 20)
res["table_cap_ms"], (cstarts, _, _) = timed(lambda: EP.episode_table(done, CAP), 20)
res["episodes"], res["episodes_cap"] = starts.numel(), cstarts.numel()
res["return_range_ms"], rr = timed(lambda: EP.return_range(replay, CAP), 20)
index = EP.EpisodeIndex.from_replay(replay)
t, _ = timed(lambda: EP.rvs_sample_batch(replay, B, index=index), BATCHES)
res["pair_batch_us"] = 1e6 * t

# the reference's way on the host: Python loops over every row, numpy draws and fancy indexing per batch
h_rew, h_done = rows[:, S].copy(), rows[:, 2 * S + 1].copy()
t0 = time.perf_counter()
h_starts, h_ends, h_len = EC.extract_done_makers(h_done)
res["numpy_table_ms"] = 1e3 * (time.perf_counter() - t0)
t0 = time.perf_counter()
h_rr = EC.return_range(h_rew, h_done, CAP)
res["numpy_return_range_ms"] = 1e3 * (time.perf_counter() - t0)
assert h_rr == rr and np.array_equal(h_ends, ends.cpu().numpy())
np.random.seed(0)
reps = 100
t0 = time.perf_counter()
for _ in range(reps):
    traj = np.random.choice(len(h_starts), B)
    s_i, g_i = EC.pairs_from_draws(h_starts, h_len, traj, np.random.rand(B), np.random.rand(B))
    obs, act, nxt = rows[s_i, :S], rows[s_i, 2 * S + 2:], rows[g_i, :S]
res["numpy_pair_batch_us"] = 1e6 * (time.perf_counter() - t0) / reps
res["table_ms"] *= 1e3
res["table_cap_ms"] *= 1e3
res["return_range_ms"] *= 1e3
print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))
