"""Cases and the numpy restatement for the hold-out partition (porl_amd/dataloader/holdout.py, csrc/partition.hpp) and
for scoring without a step (POR.evaluate / SORL.evaluate).  No reference import here: gen_holdout_golden.py records what
the reference returns for `golden_datasets()` and `score_batch()`, the tests compare this file and the device with it."""
import numpy as np

ENV_NAMES = ("antmaze-umaze-v2", "antmaze-medium-play-v2", "antmaze-large-diverse-v2", "hopper")
# the reference's three boxes and its name rule (util/util.py:220-227), restated as data
BOXES = (("umaze", (5, 10), (2, 7)), ("medium", (10, 15), (10, 15)), (None, (26, 30), (14, 18)))
N_ROWS = 1500
# scoring cases: (name, agent, layer_norm); S = 17, H = 48, L = 3, B = 50 as por_s17_h48_l3_b50
SCORE_SHAPE = dict(S=17, H=48, L=3, B=50, A=2)
SCORE_CASES = (("por", "POR", False), ("por_ln", "POR", True), ("sorl", "SORL", False), ("sorl_ln", "SORL", True))
SCORE_HYPER = {"POR": dict(tau=0.9, alpha=10.0), "SORL": dict(tau=0.9, alpha=3.0)}


def box_for(env_name):
    for key, xr, yr in BOXES:
        if key is None or key in env_name:
            return xr, yr


def held_mask(obs, x_range, y_range, cols=(0, 1)):
    """fp32 comparison, inclusive at both ends; NaN compares false, so a NaN coordinate is never held."""
    x, y = obs[:, cols[0]], obs[:, cols[1]]
    assert x.dtype == np.float32
    x_lo, x_hi, y_lo, y_hi = (np.float32(v) for v in (*x_range, *y_range))
    return (x >= x_lo) & (x <= x_hi) & (y >= y_lo) & (y <= y_hi)


def stable_partition(rows, held):
    """(out, n_kept, index): rows[~held] then rows[held], each in input order, and the original row numbers."""
    held = np.asarray(held).astype(bool)
    kept_i, held_i = np.flatnonzero(~held), np.flatnonzero(held)
    index = np.concatenate([kept_i, held_i]).astype(np.int64)
    return rows[index], int(kept_i.size), index


def generate_test_generlaization_data(dataset, env_name):
    m = held_mask(dataset["observations"], *box_for(env_name))
    return {k: v[~m] for k, v in dataset.items()}


def special_rows():
    """(name, x, y) placed at fixed rows of every golden dataset."""
    below = np.nextafter(np.float32(5), np.float32(-np.inf))
    return (("corner_lo", 5.0, 2.0), ("corner_hi", 10.0, 7.0), ("below_edge", below, 4.0), ("nan_x", np.nan, 4.0),
            ("neg_zero", -0.0, 3.0), ("medium_lo", 10.0, 10.0), ("medium_hi", 15.0, 15.0), ("large_lo", 26.0, 14.0),
            ("large_hi", 30.0, 18.0))


SPECIAL_AT = {name: 37 + 101 * k for k, (name, _, _) in enumerate(special_rows())}


def golden_datasets():
    """env name -> dict dataset: fp32 observations uniform in [0, 32)^4 with the special rows, actions, rewards,
    terminals (fp32 flags)."""
    out = {}
    for k, env in enumerate(ENV_NAMES):
        rng = np.random.default_rng(4100 + k)
        obs = rng.uniform(0, 32, size=(N_ROWS, 4)).astype(np.float32)
        for name, x, y in special_rows():
            obs[SPECIAL_AT[name], 0], obs[SPECIAL_AT[name], 1] = x, y
        out[env] = {"observations": obs,
                    "actions": rng.uniform(-1, 1, size=(N_ROWS, 2)).astype(np.float32),
                    "rewards": rng.normal(size=N_ROWS).astype(np.float32),
                    "terminals": (rng.uniform(size=N_ROWS) < 0.02).astype(np.float32)}
    return out


def score_batch(seed=71):
    """The (B, 2S+2+A) packed rows every scoring case is evaluated on."""
    from porl_amd.util.synth import make_rows
    s = SCORE_SHAPE
    return make_rows(s["B"], s["S"], s["A"], seed=seed)


def patterns(n, tile):
    """name -> bool (n,) held masks: the predicate patterns the partition is checked on."""
    i = np.arange(n)
    run = np.zeros(n, dtype=bool)
    lo = max(0, min(tile, n) - 3)
    run[lo:lo + 7] = True                       # a run across the first tile boundary (or the end of a short input)
    first, last = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    first[0], last[-1] = True, True
    return {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "first": first, "last": last,
            "alternating": i % 2 == 1, "run": run, "bernoulli": np.random.default_rng(n).uniform(size=n) < 0.3}
