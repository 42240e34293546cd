"""Times the normalisation passes (csrc/colstats.hpp) on two stores resident in HBM — 1 M x 124 (S=60, A=2; bench
config 2's rows) and 200 k x 734 (S=362, A=8):

  col_stats   `porl_col_stats` over the observation columns (0, S), queued through torch.ops.porl_hip.col_stats
  apply_      `Normalizer.apply_` with a reward scale: s, s' and r rewritten in place in one launch (mean 0, std 1, so
              the timed repetitions leave the values where they are)
  torch       the statistics as a user would otherwise write them on the same device:
              x = rows[:, :S].double(); x.mean(0); x.var(0, unbiased=False)

Each figure is the median of 5 windows of INNER = 1000 back-to-back calls between two device events, after a warm-up,
divided by INNER: a window lasts 0.1-0.6 s, far above the clock's and the scheduler's grain.  Successive calls take
COPIES = 4 equal stores in turn (2.0 / 2.3 GB together): between two visits of a store several times the 256 MB
Infinity Cache has streamed through, so every call reads from HBM.  Rates are given against the algorithmic bytes (the
span's floats, read once; read and written for apply_) and against the bytes of the 128-byte cache lines the spans
touch.  `frac_8TBps` is the algorithmic rate over 8 TB/s, `line_frac_8TBps` the touched-line rate over 8 TB/s.
One JSON line per store; DESIGN.md §4j quotes them."""
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from porl_amd.buffer.replay_buffer import PackedReplay  # noqa: E402
from porl_amd.dataloader import Normalizer, column_stats  # noqa: E402
import porl_amd.ops  # noqa: E402,F401

REPS, INNER, COPIES, LINE, PEAK = 5, 1000, 4, 128, 8e12
dev = torch.device("cuda", 0)


def device_ms(fn):
    """`fn(i)` is call number i; it picks store i % COPIES."""
    for i in range(2 * COPIES):
        fn(i)
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(INNER):
            fn(i)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / INNER)
    return statistics.median(times)


def line_bytes(n, width, spans):
    """Bytes of the distinct 128-byte lines that columns `spans` of n dense rows of `width` floats touch (a 128-byte
    aligned base): the pattern repeats every LINE / gcd(pitch, LINE) rows."""
    pitch = 4 * width
    period = LINE // math.gcd(pitch, LINE)
    lines = set()
    for r in range(period):
        for c0, c in spans:
            lo, hi = r * pitch + 4 * c0, r * pitch + 4 * (c0 + c) - 1
            lines.update(range(lo // LINE, hi // LINE + 1))
    return len(lines) * LINE * n / period


def rate(nbytes, ms):
    return round(nbytes / ms / 1e6, 1)                              # GB/s


for N, S, A in ((1_000_000, 60, 2), (200_000, 362, 8)):
    W = 2 * S + 2 + A
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = torch.randn(N, W, device=dev, generator=gen)
    rows[:, 2 * S + 1] = (torch.arange(N, device=dev) % 1000 == 999).float()
    replays = [PackedReplay(rows.clone() if k else rows, S, A, dev) for k in range(COPIES)]
    replay = replays[0]
    res = {"rows": N, "width": W, "obs_dim": S}

    ms = device_ms(lambda i: torch.ops.porl_hip.col_stats(replays[i % COPIES].rows, 0, S))
    alg, lines = 4.0 * N * S, line_bytes(N, W, [(0, S)])
    res.update(col_stats_ms=ms, col_stats_rows_per_s=round(N / ms * 1e3), col_stats_GBps=rate(alg, ms),
               col_stats_line_GBps=rate(lines, ms), col_stats_frac_8TBps=round(alg / (ms * 1e-3) / PEAK, 4),
               col_stats_line_frac_8TBps=round(lines / (ms * 1e-3) / PEAK, 4))

    def torch_way(i=0):
        x = replays[i % COPIES].rows[:, :S].double()
        return x.mean(0), x.var(0, unbiased=False)

    tms = device_ms(torch_way)
    res.update(torch_double_mean_var_ms=tms, torch_over_col_stats=round(tms / ms, 2))
    st = column_stats(replay)
    tm, tv = torch_way()
    res["max_abs_mean_diff_vs_torch"] = float(np.abs(st.mean - tm.cpu().numpy()).max())
    res["max_rel_var_diff_vs_torch"] = float(np.abs(st.var / tv.cpu().numpy() - 1).max())

    norm = Normalizer(torch.zeros(S), torch.ones(S)).to(dev).with_reward_scale(0.0, 1.0, 1.0)
    ms = device_ms(lambda i: norm.apply_(replays[i % COPIES]))
    assert all(torch.equal(r.rows, rows) for r in replays[1:])      # (x - 0) / 1 and r / 1 * 1: the stores are where they were
    spans = [(0, S), (S, 1), (S + 1, S)]
    alg, lines = 2 * 4.0 * N * (2 * S + 1), 2 * line_bytes(N, W, spans)
    res.update(apply_ms=ms, apply_rows_per_s=round(N / ms * 1e3), apply_GBps=rate(alg, ms), apply_line_GBps=rate(lines, ms),
               apply_frac_8TBps=round(alg / (ms * 1e-3) / PEAK, 4))
    print(json.dumps({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
    del rows, replay, replays
    torch.cuda.empty_cache()
