"""The normalisation passes restated in numpy (porl_amd/dataloader/normalize.py, csrc/colstats.hpp), the column cases and
bounds of tests/test_normalize_host.py / test_normalize_gpu.py, and the scripted environment of
tests/test_evaluate_loops_gpu.py.  No GPU, no torch.

Oracle.  `oracle(x)`: mean = fsum(x) / n, M2 = fsum((x - mean)^2), min, max — math.fsum adds exactly and rounds once.

Bounds (derived, not measured).  With u = 2^-53, fp64 summation of N exactly represented fp32 values errs by at most
(N - 1) u sum|x|, so the mean by at most N u mean|x|: the tests allow |d mean| <= 4 N u mean|x|.  M2 is a sum of N
non-negative terms each carrying a few roundings, plus the d^2 n_a n_b / n terms of the merges (a handful of roundings
per level): |d var| <= 64 N u var_oracle.  min and max are exact.  A constant column has var_oracle == 0: only 0.0 passes.
"""
import math

import numpy as np

try:
    from . import episode_cases                                    # as tests/helpers/normalize_cases
except ImportError:
    import episode_cases                                           # run from this directory (gen_normalize_golden.py)

U64 = 2.0 ** -53
CASES = ("gauss", "scaled", "offset", "const", "flags", "nan1", "inf1")
FINITE = CASES[:5]
HOST_N = 70001


def column(case, n, rng):
    """One fp32 column of `n` values; every value is exactly representable in fp32 by construction."""
    if case == "gauss":
        return rng.standard_normal(n).astype(np.float32)
    if case == "scaled":
        return (np.float32(1e3) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    if case == "offset":                                           # 4096 + k 2^-9: 13 + 9 bits, exact in fp32
        return (4096.0 + rng.integers(-8, 9, size=n) * 2.0 ** -9).astype(np.float32)
    if case == "const":
        return np.full(n, np.float32(0.3), dtype=np.float32)
    if case == "flags":
        return (rng.random(n) < 0.05).astype(np.float32)
    x = rng.standard_normal(n).astype(np.float32)
    x[int(rng.integers(0, n))] = np.float32(np.nan) if case == "nan1" else np.float32(np.inf)
    return x


def interleaved(n, width, span, seed):
    """(rows (n, width) fp32, case name per span column): the seven cases cycle across the span's columns; columns
    outside the span hold N(0, 1) with a NaN and an inf sprinkled in (they must not be read)."""
    rng = np.random.default_rng(seed)
    col0, c = span
    rows = rng.standard_normal((n, width)).astype(np.float32)
    if col0 > 0:
        rows[0, col0 - 1] = np.nan
    if col0 + c < width:
        rows[n - 1, col0 + c] = np.inf
    names = [CASES[j % len(CASES)] for j in range(c)]
    for j, name in enumerate(names):
        rows[:, col0 + j] = column(name, n, rng)
    return rows, names


def oracle(x):
    """(mean, M2, min, max) of one column in fp64; a NaN gives four NaNs (numpy's mean / min / max)."""
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).any():
        return (np.nan,) * 4
    if np.isinf(x).any():
        with np.errstate(invalid="ignore"):
            return float(np.mean(x)), np.nan, float(x.min()), float(x.max())
    mean = math.fsum(x) / x.size
    e = x - mean
    return mean, math.fsum(e * e), float(x.min()), float(x.max())


def bounds(x, n=None):
    """(bound on |d mean|, bound on |d var|) for a finite column."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size if n is None else n
    mean, m2, _, _ = oracle(x)
    return 4 * n * U64 * (math.fsum(np.abs(x)) / x.size), 64 * n * U64 * (m2 / x.size)


def merge(a, b):
    """(n, mean, M2, min, max) of two disjoint samples: d = mean_b - mean_a, mean = mean_a + d n_b / n,
    M2 = M2_a + M2_b + d^2 n_a n_b / n."""
    na, ma, sa, lo_a, hi_a = a
    nb, mb, sb, lo_b, hi_b = b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    r = nb / n
    d = mb - ma
    return n, ma + d * r, sa + sb + d * d * (na * r), min(lo_a, lo_b), max(hi_a, hi_b)


def tile_stats(x):
    """One tile in plain fp64 numpy (pairwise summation, two passes) — what a block computes, up to association."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.sum() / x.size
    e = x - mean
    return x.size, float(mean), float((e * e).sum()), float(x.min()), float(x.max())


def tile_merged(x, tile, sweep):
    """The kernels' structure on one column: tiles of `tile` rows, then groups of `sweep` consecutive partials folded
    left to right, level after level."""
    parts = [tile_stats(x[i:i + tile]) for i in range(0, len(x), tile)]
    while len(parts) > 1:
        nxt = []
        for g in range(0, len(parts), sweep):
            acc = parts[g]
            for p in parts[g + 1:g + sweep]:
                acc = merge(acc, p)
            nxt.append(acc)
        parts = nxt
    return parts[0]


def one_pass(x):
    """NEGATIVE control: the sum x^2, sum x form in fp64.  -> (mean, var)."""
    x = np.asarray(x, dtype=np.float64)
    s, q = 0.0, 0.0
    for chunk in np.array_split(x, max(1, x.size // 512)):         # any association: the cancellation is in the formula
        s += float(chunk.sum())
        q += float((chunk * chunk).sum())
    mean = s / x.size
    return mean, q / x.size - mean * mean


def fp32_accumulation(x):
    """NEGATIVE control: numpy's fp32 route.  -> (mean, var) as computed in fp32."""
    x = np.asarray(x, dtype=np.float32)
    return float(x.mean(dtype=np.float32)), float(x.var(dtype=np.float32))


def normalizer_from_stats(n, mean, m2, eps=1e-3):
    """(mean32, std32) = (fp32(mean64), fp32(sqrt(M2 / n) + eps))."""
    mean, m2 = np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64)
    return mean.astype(np.float32), (np.sqrt(m2 / n) + eps).astype(np.float32)


def affine(rows, spans, shift, div, mul=None):
    """fp32, one rounding per operation: out[:, c0+j] = fl(fl(rows[:, c0+j] - shift[p0+j]) / div[p0+j]), then
    fl(. * mul[p0+j]) where flags & 1.  Other columns are returned as they are (bit for bit)."""
    out = np.array(rows, dtype=np.float32, copy=True)
    shift, div = np.asarray(shift, dtype=np.float32), np.asarray(div, dtype=np.float32)
    with np.errstate(all="ignore"):
        for c0, c, p0, flags in spans:
            x = rows[:, c0:c0 + c].astype(np.float32)
            y = ((x - shift[p0:p0 + c]).astype(np.float32) / div[p0:p0 + c]).astype(np.float32)
            if flags & 1:
                y = (y * np.asarray(mul, dtype=np.float32)[p0:p0 + c]).astype(np.float32)
            out[:, c0:c0 + c] = y
    return out


def reciprocal_pairs(count, seed=0):
    """(x, d) fp32 pairs, d no power of two, with fl(x * fl(1 / d)) != fl(x / d): a division turned into a reciprocal
    multiplication shows on every one of them."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 4.0, size=64 * count).astype(np.float32)
    d = rng.uniform(1.1, 7.9, size=64 * count).astype(np.float32)
    frac, _ = np.frexp(d)
    keep = ((x * (np.float32(1) / d).astype(np.float32)).astype(np.float32) != (x / d).astype(np.float32)) & (frac != 0.5)
    x, d = x[keep][:count], d[keep][:count]
    assert x.size >= min(count, 100), f"found only {x.size} pairs"
    return x, d


def normalize_rows(rows, obs_dim, stats_rows=None, max_episode_steps=None, eps=1e-3):
    """What normalize_dataset leaves in a packed [s | r | s' | d | a] store -> (rows, mean32, std32, reward_div,
    reward_mul): statistics of the observation columns of `stats_rows` (default `rows`) by the oracle."""
    S = obs_dim
    src = rows if stats_rows is None else stats_rows
    st = [oracle(src[:, j]) for j in range(S)]
    mean32, std32 = normalizer_from_stats(src.shape[0], [s[0] for s in st], [s[1] for s in st], eps)
    spans = [(0, S, 0, 0), (S + 1, S, 0, 0)]
    shift, div, mul = np.append(mean32, np.float32(0)), np.append(std32, np.float32(1)), np.ones(S + 1, dtype=np.float32)
    rdiv = rmul = None
    if max_episode_steps is not None:
        lo, hi = episode_cases.return_range(rows[:, S], rows[:, 2 * S + 1], max_episode_steps)
        rdiv, rmul = np.float32(hi - lo), np.float32(max_episode_steps)
        div[S], mul[S] = rdiv, rmul
        spans.append((S, 1, S, 1))
    return affine(rows, spans, shift, div, mul), mean32, std32, rdiv, rmul


def packed_rows(n, obs_dim, act_dim, seed, lo=-3.0, hi=3.0, done_every=37):
    """[s | r | s' | d | a] rows: U(lo, hi) observations, N(0, 1) rewards, a done flag every `done_every` rows."""
    rng = np.random.default_rng(seed)
    S, A = obs_dim, act_dim
    rows = np.empty((n, 2 * S + 2 + A), dtype=np.float32)
    rows[:, :S] = rng.uniform(lo, hi, size=(n, S))
    rows[:, S] = rng.standard_normal(n)
    rows[:, S + 1:2 * S + 1] = rng.uniform(lo, hi, size=(n, S))
    rows[:, 2 * S + 1] = (np.arange(n) % done_every == done_every - 1)
    rows[:, 2 * S + 2:] = rng.uniform(-1, 1, size=(n, A))
    return rows


# ---- the scripted environment of the evaluator tests ---------------------------------------------------------------------
EVAL_S, EVAL_A, EVAL_STEPS, EVAL_H, EVAL_L = 6, 2, 12, 32, 2
EVAL_GOAL = (1.5, -0.75)


def eval_observations():
    """The recorded 13 observations (reset + 12 steps), float64 as a gym environment returns them."""
    return np.random.default_rng(2024).uniform(-2.0, 2.0, size=(EVAL_STEPS + 1, EVAL_S))


def eval_mean_std():
    rng = np.random.default_rng(2025)
    return rng.uniform(-0.5, 0.5, size=EVAL_S).astype(np.float32), rng.uniform(0.5, 2.0, size=EVAL_S).astype(np.float32)


class ScriptedEnv:
    """Observations are a recorded sequence independent of the action (closed-loop error cannot amplify); the reward
    is -|a|^2; `done` comes with step 12.  `actions` records what the loop sent."""

    target_goal = EVAL_GOAL

    def __init__(self, observations=None):
        self.obs = eval_observations() if observations is None else np.asarray(observations)
        self.t = 0
        self.actions = []

    def reset(self):
        self.t = 0
        self.actions = []
        return self.obs[0].copy()

    def step(self, action):
        a = np.asarray(action, dtype=np.float64)
        self.actions.append(np.array(action, copy=True))
        self.t += 1
        return self.obs[self.t].copy(), -float((a * a).sum()), self.t >= len(self.obs) - 1, {}
