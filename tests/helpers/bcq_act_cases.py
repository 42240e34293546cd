"""numpy restatement of the BCQ-constrained select rule (csrc/bcq_act.hpp) and the case grid its tests walk.

Two paths.  The fp32 path restates the kernel's expressions in its order — softmax by a sequential maximum, a sequential
sum and one division, the mask p > threshold, the arg-max of q + (mask - 1) * 1e10 with the first maximum and a NaN
counting as the maximum; given the same mask it must give the device's action bit for bit (no transcendental is left in
it).  The fp64 path is the oracle of the mask: the device's expf may differ from numpy's by an ulp, so a mask bit is pinned
only on rows where no fp64 probability lies within MARGIN of the threshold.  The fp32 softmax takes at most A + 4
roundings of 2^-24 on values <= 1 — 4e-6 at A = 64 — so MARGIN = 1e-5 covers it.

Every case plants four rows when it has room for them (n >= 255) and the threshold allows the row to exist:
  ROW_TIE   the two largest action values are equal (exact tie, both allowed when the mask allows them);
  ROW_NAN   one action value is NaN: v = NaN + (mask - 1) * 1e10 is NaN whether the action is allowed or not, and a NaN
            counts as the maximum (torch.argmax over v), so this row takes that action under every threshold;
  ROW_NONE  uniform logits with 1 / A below the threshold: every action is masked, action values inside (-512, 512);
  ROW_ONE   one logit 12 above the rest with the threshold between the two probabilities: exactly one action allowed,
            and it is not the one the plain arg-max would take."""
import itertools

import numpy as np

ACTIONS = (1, 2, 5, 64)
ROWS = (1, 255, 257, 600)
THRESHOLDS = (0.0, 0.1, 0.3, 0.99)
SIGMAS = (0.5, 3.0)
MARGIN = 1e-5
ROW_TIE, ROW_NAN, ROW_NONE, ROW_ONE = 3, 7, 11, 13


def cases():
    return list(itertools.product(ACTIONS, ROWS, SIGMAS))


def grid():
    return list(itertools.product(ACTIONS, ROWS, SIGMAS, THRESHOLDS))


def _seed(A, n, sigma):
    return 1000 * A + 10 * n + int(2 * sigma)


def has_none(A, threshold):
    """An all-masked row exists: the uniform row's probability 1 / A lies well below the threshold."""
    return 1.0 / A < threshold - 1e-3


def has_one(A, threshold):
    """A row with exactly one allowed action exists: e^-12 / (1 + (A - 1) e^-12) < threshold < 1 / (1 + (A - 1) e^-12)."""
    lo = np.exp(-12.0) / (1.0 + (A - 1) * np.exp(-12.0))
    return A >= 2 and lo < threshold - 1e-3 and threshold + 1e-3 < 1.0 / (1.0 + (A - 1) * np.exp(-12.0))


def nan_column(A):
    return A // 2


def tables(A, n, sigma, threshold):
    """(q, z): action values and behaviour logits (n, A) fp32 of one case, the planted rows included."""
    rng = np.random.default_rng(_seed(A, n, sigma))
    z = (rng.standard_normal((n, A)) * sigma).astype(np.float32)
    q = (rng.standard_normal((n, A)) * 2.0).astype(np.float32)
    if n >= 255:
        if A >= 2:
            top = int(np.argmax(q[ROW_TIE]))
            q[ROW_TIE, (top + 1) % A] = q[ROW_TIE, top]
        q[ROW_NAN, nan_column(A)] = np.nan
        if has_none(A, threshold):
            z[ROW_NONE] = np.float32(0.25)
            q[ROW_NONE] = rng.uniform(-500.0, 500.0, A).astype(np.float32)
        if has_one(A, threshold):
            best = int(np.argmax(q[ROW_ONE]))
            z[ROW_ONE] = np.float32(-1.0)
            z[ROW_ONE, (best + 1) % A] = np.float32(11.0)
    return q, z


def probs_f64(z):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def near(z, threshold, margin=MARGIN):
    """Rows with some fp64 probability within `margin` of the threshold: their mask is not pinned.  Threshold 0 is the one
    place where the absolute margin says nothing — at sigma 3 nearly every row of 64 actions has a probability below 1e-5,
    all of them far above 0 in fp32's own terms: p_j > 0 holds in fp32 exactly when expf(z_j - mx) does not underflow (se >= 1
    is finite, the quotient of two normal numbers of this size is not 0).  So at threshold 0 a row is left out only when some
    z_j - mx lies below -80 (fp32's exp reaches 0 past -103), which asks more of the device than the margin would."""
    if threshold == 0.0:
        z = z.astype(np.float64)
        return ((z - z.max(axis=1, keepdims=True)) < -80.0).any(axis=1)
    return (np.abs(probs_f64(z) - threshold) <= margin).any(axis=1)


def mask_f64(z, threshold):
    return (probs_f64(z) > threshold).astype(np.float32)


def mask_f32(z, threshold):
    """The kernel's softmax in its order, in fp32: sequential fmaxf, sequential sum of expf, one division per action."""
    z = z.astype(np.float32)
    n, A = z.shape
    mx = np.full(n, -np.inf, dtype=np.float32)
    for j in range(A):
        mx = np.fmax(mx, z[:, j])
    se = np.zeros(n, dtype=np.float32)
    for j in range(A):
        se = (se + np.exp(z[:, j] - mx, dtype=np.float32)).astype(np.float32)
    p = np.stack([np.exp(z[:, j] - mx, dtype=np.float32) / se for j in range(A)], axis=1).astype(np.float32)
    return (p > np.float32(threshold)).astype(np.float32)


def select(q, mask):
    """Greedy action per row from action values and a 0 / 1 mask, the kernel's expression and comparison in fp32."""
    q, mask = q.astype(np.float32), mask.astype(np.float32)
    with np.errstate(invalid="ignore"):
        v = (q + ((mask - np.float32(1.0)) * np.float32(1e10)).astype(np.float32)).astype(np.float32)
    n, A = v.shape
    best, pick = v[:, 0].copy(), np.zeros(n, dtype=np.int64)
    for j in range(1, A):
        vj = v[:, j]
        with np.errstate(invalid="ignore"):
            take = (best == best) & ((vj > best) | (vj != vj))
        best = np.where(take, vj, best)
        pick = np.where(take, j, pick)
    return pick, v
