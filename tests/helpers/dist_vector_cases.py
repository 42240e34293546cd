"""What porl_dist_select computes (csrc/dist_act.hpp), in numpy: the fp64 oracle of the action values of a distributional
head, the fp32 restatement in the kernel's summation order, and the grid of shapes the tests run.

A row holds A x NS floats, action a in columns [a * NS, (a + 1) * NS).
  QR   value = mean of the NS quantiles
  C51  value = sum_n softmax(row[a, :])_n support[n]      (support: the caller's torch.linspace(v_min, v_max, NS), fp32)
The kernel sums with one 64-lane wave per row: lane l adds elements l, l + 64, ... in ascending order, then the xor
butterfly 32, 16, .., 1 combines the lanes (every lane ends with the same bits)."""
import numpy as np

QR, C51 = 0, 1
V_MAX = 10.0                                     # C51 support: [-10, 10]
SIGMAS = (1.0, 3.0)                              # logits / quantiles are drawn N(0, sigma): logits()
QR_GRID = ((5, 51), (3, 1), (7, 65), (1, 4), (64, 4), (5, 256))
C51_GRID = ((5, 51), (3, 2), (7, 65), (64, 4), (5, 256), (1, 51))
N_ROWS = 1029                                    # 257 blocks of four rows plus one wave
GAP = 1e-3                                       # rows whose two best fp64 values are closer are not asked for their arg-max


def cases():
    """(kind, A, NS, sigma) over both grids."""
    return [(kind, A, NS, s) for kind, grid in ((QR, QR_GRID), (C51, C51_GRID)) for A, NS in grid for s in SIGMAS]


def logits(kind, A, NS, sigma, n=N_ROWS):
    """(n, A * NS) float32, every element N(0, sigma): sigma (u_a + e_aj) / sqrt(2) with u per action and e per element,
    both standard normal.  The part an action's elements share is what the quantiles of one return distribution have in
    common, their location.  Elements drawn independently would give quantile means of spread sigma / sqrt(NS), and the two
    best of them then lie within GAP of each other in up to 2 % of the rows ((7, 65) and (5, 256) at sigma 1: 1.7 %, 1.9 % of
    1 029 rows, as do C51's (64, 4) at sigma 3: 1.2 %); with the shared part no case exceeds 0.5 %."""
    rng = np.random.default_rng([kind, A, NS, int(sigma), n])
    u, e = rng.standard_normal((n, A, 1)), rng.standard_normal((n, A, NS))
    return (sigma * (u + e) / np.sqrt(2.0)).reshape(n, A * NS).astype(np.float32)


def oracle(kind, z, A, NS, support=None):
    """(n, A) fp64 action values of the fp32 rows z."""
    x = z.astype(np.float64).reshape(z.shape[0], A, NS)
    if kind == QR:
        return x.mean(axis=2)
    e = np.exp(x - x.max(axis=2, keepdims=True))
    p = e / e.sum(axis=2, keepdims=True)
    return (p * support.astype(np.float64)[None, None, :]).sum(axis=2)


def top2_gap(values):
    """Per row: best minus second-best value (inf with one action)."""
    if values.shape[1] < 2:
        return np.full(values.shape[0], np.inf)
    s = np.sort(values, axis=1)
    return s[:, -1] - s[:, -2]


def _wave_sum(x, fill=0.0):
    """fp32 sum over the last axis (length NS) in the wave's order; x: (..., NS) float32."""
    NS = x.shape[-1]
    part = np.full(x.shape[:-1] + (64,), fill, dtype=np.float32)
    for j0 in range(0, NS, 64):                                  # lane l: elements l, l + 64, ... in ascending order
        w = min(64, NS - j0)
        part[..., :w] = part[..., :w] + x[..., j0:j0 + w]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[..., lanes ^ o]
    return part[..., 0]


def values_f32(kind, z, A, NS, support=None):
    """(n, A) float32: the kernel's arithmetic, operation for operation (numpy's expf / logf for the device's)."""
    x = z.reshape(z.shape[0], A, NS).astype(np.float32)
    if kind == QR:
        return (_wave_sum(x) / np.float32(NS)).astype(np.float32)
    mx = x.max(axis=2, keepdims=True)
    se = _wave_sum(np.exp(x - mx))
    lse = (mx[..., 0] + np.log(se)).astype(np.float32)
    return _wave_sum(np.exp(x - lse[..., None]) * support.astype(np.float32)[None, None, :]).astype(np.float32)
