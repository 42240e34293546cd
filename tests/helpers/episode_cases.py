"""Numpy restatement of the reference's trajectory-level dataset functions (util/util.py:67-138), of the counter-based
generator of porl_hindsight_pairs, and the case generators the episode tests share.

Nothing here imports the reference or the product: tests/helpers/gen_episodes_golden.py records what the reference
itself returns (tests/golden/episodes_ref.npz), and tests/test_episodes_host.py checks this restatement against it.
"""
import numpy as np

CAPS = (1, 2, 7, 1000)
M64 = (1 << 64) - 1


# ---- the reference, restated ------------------------------------------------------------------------------------------
def flags_set(dones):
    """A flag is set iff it is != 0.0: NaN set, -0.0 clear (np.where(dones) / `if d`)."""
    return np.asarray(dones, dtype=np.float32) != 0


def extract_done_makers(dones):
    """util/util.py:83-87, except that no set flag gives three empty arrays (the reference returns starts = [0] with
    empty ends, which its only caller cannot index)."""
    ends = np.flatnonzero(flags_set(dones)).astype(np.int64)
    if ends.size == 0:
        return ends, ends.copy(), ends.copy()
    starts = np.concatenate(([0], ends[:-1] + 1)).astype(np.int64)
    return starts, ends, ends - starts + 1


def capped_table(dones, cap):
    """(starts, ends, trailing) of the episodes return_range closes (util/util.py:67-80): at a set flag or when ep_len
    reaches `cap` (cap None or 0: flags only).  Row-by-row walk, as the reference does it."""
    s = flags_set(dones)
    starts, ends, a, ep_len = [], [], 0, 0
    for i in range(s.size):
        ep_len += 1
        if s[i] or (cap and ep_len == cap):
            starts.append(a)
            ends.append(i)
            a, ep_len = i + 1, 0
    return np.array(starts, dtype=np.int64), np.array(ends, dtype=np.int64), ep_len


def episode_returns(rewards, dones, cap):
    """The two lists of return_range: returns as Python floats added in row order, lengths with the trailing count."""
    starts, ends, trailing = capped_table(dones, cap)
    r = np.asarray(rewards, dtype=np.float32)
    returns = []
    for a, b in zip(starts, ends):
        acc = 0.
        for x in r[a:b + 1]:
            acc += float(x)
        returns.append(acc)
    return np.array(returns, dtype=np.float64), np.concatenate([ends - starts + 1, [trailing]]).astype(np.int64)


def return_range(rewards, dones, cap):
    returns, _ = episode_returns(rewards, dones, cap)
    return min(returns.tolist()), max(returns.tolist())


def pairs_from_draws(starts, lengths, traj, u1, u2):
    """util/util.py:101-114 on given draws."""
    t1 = np.floor(u1 * (lengths[traj] - 1)).astype(np.int64)
    t2 = np.floor(u2 * lengths[traj]).astype(np.int64)
    return starts[traj] + np.minimum(t1, t2), starts[traj] + np.maximum(t1, t2)


# ---- the generator, restated --------------------------------------------------------------------------------------------
def sm64(z):
    """splitmix64's output function on Python ints."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def device_draws(seed, step, batch, n_episodes):
    """(traj int64, u1, u2 fp64) of porl_hindsight_pairs: key = sm64(seed ^ sm64(step)), x_s(i) = sm64(key ^ sm64(3 i + s)),
    traj = mulhi64(x_0, E), u = (x >> 11) * 2^-53."""
    key = sm64((seed & M64) ^ sm64(step & M64))
    traj = np.empty(batch, dtype=np.int64)
    u1 = np.empty(batch, dtype=np.float64)
    u2 = np.empty(batch, dtype=np.float64)
    for i in range(batch):
        x = [sm64(key ^ sm64(3 * i + s)) for s in range(3)]
        traj[i] = (x[0] * n_episodes) >> 64
        u1[i] = (x[1] >> 11) * 2.0 ** -53
        u2[i] = (x[2] >> 11) * 2.0 ** -53
    return traj, u1, u2


# ---- cases ------------------------------------------------------------------------------------------------------------------
def golden_vectors():
    """name -> (rewards fp32, dones fp32), N <= 5000: what gen_episodes_golden.py feeds the reference."""
    rng = np.random.default_rng(20240611)
    out = {}

    def rew(n):
        return (rng.standard_normal(n) * 1e3).astype(np.float32)

    n = 5000
    out["random"] = (rew(n), (rng.random(n) < 1 / 40).astype(np.float32))
    out["dense"] = (rew(777), (rng.random(777) < 1 / 3).astype(np.float32))
    out["all_set"] = (rew(300), np.ones(300, dtype=np.float32))
    d = np.zeros(1000, dtype=np.float32); d[0] = 1
    out["first_only"] = (rew(1000), d)
    d = np.zeros(1000, dtype=np.float32); d[-1] = 1
    out["last_only"] = (rew(1000), d)
    d = (rng.random(2000) < 1 / 100).astype(np.float32); d[137] = np.nan; d[1999] = 1
    out["nan_flag"] = (rew(2000), d)
    d = (rng.random(2000) < 1 / 100).astype(np.float32); d[d == 0] = -0.0; d[55] = 2.5; d[1200] = -1.0
    out["neg_zero"] = (rew(2000), d)
    return out


def flag_pattern(kind, n, seed):
    rng = np.random.default_rng(seed)
    d = np.zeros(n, dtype=np.float32)
    if kind == "third":
        d[rng.random(n) < 1 / 3] = 1
    elif kind == "sparse":
        d[rng.random(n) < 1 / 500] = 1
    elif kind == "all":
        d[:] = 1
    elif kind == "last":
        d[-1] = 1
    elif kind == "first":
        d[0] = 1
    elif kind != "none":
        raise ValueError(kind)
    return d


PATTERNS = ("third", "sparse", "all", "none", "last", "first")

# (case, vector whose flags delimit the trajectories, np.random.seed, batch, vector whose flags sit in 'terminals' when
# the delimiting ones come as 'timeouts' — None: the delimiting flags ARE the terminals)
PAIR_CASES = (
    ("random_s1", "random", 1, 256, None),
    ("dense_s2", "dense", 2, 257, None),
    ("one_row_episodes", "all_set", 3, 64, None),
    ("nan_flag_s4", "nan_flag", 4, 128, None),
    ("timeouts_over_terminals", "neg_zero", 5, 128, "nan_flag"),
)
