"""Seeded cases of the BCQ behaviour-mask kernel (porl_qnet_bcq_mask), shared by the CPU margin check
(tests/test_bcq_rows.py) and the GPU comparison (tests/test_bcq_rows_gpu.py): behaviour-policy parameters, a 200-row
next_states array, a non-monotone index slice, a threshold inside the spread of the probabilities, and the fp64 numpy
forward both sides judge by."""
import itertools

import numpy as np

N_ROWS = 200
BATCHES, ACTIONS, STATES = (1, 31, 33, 65), (2, 3, 6, 33), (3, 10, 60)
# hidden sizes: the reference's default, one layer, three layers (one-launch kernel), one 256-wide layer (multi-launch)
HIDDEN = {"default": [64, 128], "h48": [48], "h3": [64, 128, 64], "wide": [256]}
MARGIN = 1e-5


def shapes(hidden_key):
    """(B, A, S) of every case: the full grid on the default network, a covering subset on the others."""
    grid = list(itertools.product(BATCHES, ACTIONS, STATES))
    return grid if hidden_key == "default" else [g for i, g in enumerate(grid) if i % 5 == 0 or g == (65, 33, 60)]


def make(hidden_key, B, A, S):
    hidden = HIDDEN[hidden_key]
    rng = np.random.default_rng(1000 * B + 10 * A + S + 7 * len(hidden) + hidden[0])
    dims = [S] + list(hidden) + [A]
    params = {}
    for l in range(len(dims) - 1):
        # (gain 1.6: logits of a few units' spread, so the probabilities straddle the threshold)
        params[f"network.{2 * l}.weight"] = (1.6 * rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32)
        params[f"network.{2 * l}.bias"] = (0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32)
    next_states = (1.5 * rng.standard_normal((N_ROWS, S))).astype(np.float32)
    idx = rng.permutation(N_ROWS)[:B].astype(np.int64)
    return dict(hidden=hidden, params=params, next_states=next_states, idx=idx, threshold=float(np.float32(1.0 / A)))


def probs64(case):
    """fp64 softmax(behaviour MLP(next_states[idx])) -> (B, A)."""
    h = case["next_states"][case["idx"]].astype(np.float64)
    n = len(case["hidden"]) + 1
    for l in range(n):
        h = h @ case["params"][f"network.{2 * l}.weight"].astype(np.float64).T + case["params"][f"network.{2 * l}.bias"]
        if l < n - 1:
            h = np.maximum(h, 0.0)
    e = np.exp(h - h.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def decided(case):
    """(mask the fp64 probabilities give, entries at least MARGIN away from the threshold)."""
    p = probs64(case)
    return (p > case["threshold"]).astype(np.float32), np.abs(p - case["threshold"]) >= MARGIN
