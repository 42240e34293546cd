"""Times the hold-out split (csrc/partition.hpp) on 1 M packed rows of S=60, A=2 resident in HBM: `partition_rows` in the
box form (kept and held part from one copy, the read-back of K included), the torch way it replaces on the same device
(`m` from torch comparisons, `rows[~m]`, `rows[m]`), and the numpy restatement of the reference's function on the same rows on
the host (tests/helpers/holdout_cases.py).  Device times are medians of 5 by device events after a warm-up.
One JSON line; DESIGN.md §4i quotes it."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from helpers import holdout_cases as HC  # noqa: E402
from porl_amd.dataloader.holdout import partition_rows  # noqa: E402

S, A, N, REPS = 60, 2, 1_000_000, 5
X_RANGE, Y_RANGE = (5, 10), (2, 7)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
rows = rng.standard_normal((N, 2 * S + 2 + A)).astype(np.float32)
rows[:, :2] = rng.uniform(0, 32, size=(N, 2)).astype(np.float32)
drows = torch.from_numpy(rows).to(dev)


def device_ms(fn):
    fn()
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), out


def torch_way():
    x, y = drows[:, 0], drows[:, 1]
    m = (x >= X_RANGE[0]) & (x <= X_RANGE[1]) & (y >= Y_RANGE[0]) & (y <= Y_RANGE[1])
    return drows[~m], drows[m]


res = {"rows": N, "obs_dim": S, "act_dim": A, "row_bytes": 4 * rows.shape[1]}
res["partition_ms"], part = device_ms(lambda: partition_rows(drows, x_range=X_RANGE, y_range=Y_RANGE))
res["torch_mask_index_ms"], (t_kept, t_held) = device_ms(torch_way)
assert torch.equal(part.kept, t_kept) and torch.equal(part.held, t_held)
res["kept"], res["held"] = part.n_kept, N - part.n_kept
res["partition_GBps"] = round(2 * rows.nbytes / res["partition_ms"] / 1e6, 1)

# the same split on the host: the numpy restatement of the reference's function on its dict of arrays
ds = {"observations": rows[:, :S].copy(), "rewards": rows[:, S].copy(), "next_observations": rows[:, S + 1:2 * S + 1].copy(),
      "terminals": rows[:, 2 * S + 1].copy(), "actions": rows[:, 2 * S + 2:].copy()}
t0 = time.perf_counter()
held = HC.held_mask(ds["observations"], X_RANGE, Y_RANGE)
host = {k: v[~held] for k, v in ds.items()}
res["numpy_host_ms"] = 1e3 * (time.perf_counter() - t0)
assert host["rewards"].size == part.n_kept
print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))
