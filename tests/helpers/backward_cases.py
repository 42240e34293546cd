"""Cases of the IQL engine's two backward phases (porl_iql_value_backward, porl_iql_policy_backward and the
policy-only forward half): tests/test_backward_cases.py checks them on the CPU, tests/test_backward_gpu.py runs them on
the device.  numpy only, no device use.

`CASES` are the engine configurations of tests/helpers/forward_cases.py (same parameters, `fill`) plus two
backward-only configurations; `RUNS` is the grid: (case, batch, tune) triples that reach every tile walk of
csrc/skinny.hpp and every loop trip of the head / NLL kernels, each run under weight_mode 0 and 1.  `skn_split`,
`skinny_kernels` and `splits` restate the host code's choices (iql_api.inc) in Python.

Inputs.  A batch is the first B DECIDED rows of a seeded pool.  The only discontinuities of the two phases are the
ReLU gates of the nets that receive gradients (the online twins on s, the policy on s; min, the expectile weight times u
and the weight clip are continuous): a pool row is decided when, in fp64, every hidden pre-activation of those three
nets (after LayerNorm's affine where there is one) has |z| >= MARGIN.  No comparison ever has to leave a row out.
log_std is overwritten per case with entries below -5, above 2, exactly -5.0 and exactly 2.0 (as many of the four as D
holds, see `log_std_for`); the regression target is the fp64 policy mean plus a multiple of sigma per column, |z| in
[0.4, 1.6], so that no column of d/dmean hides the others by more than 1 / sigma_min; the output units of the columns with
sigma = e^-5 are scaled down (see `params`) so that z there is not one amplified rounding of the mean.

Reference and bar.  `backward64` is the yardstick, `backward32` the same formulas in numpy fp32; the error of a tensor is
max |got - ref64| / max |ref64| over that tensor, its bar max(BAR_FLOOR, BAR_FACTOR x e32) with forward_cases' constants.
A tensor whose fp64 reference is exactly zero must come back exactly zero.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from helpers import forward_cases as FC
from oracle import por_oracle as O

MARGIN = 1e-4                       # qstep_cases.MARGIN
TAU, DISCOUNT = 0.7, 0.99
# weight_mode 0: min(exp(adv / alpha), 100) clips at adv > 2.30; weight_mode 1: min(exp(alpha * adv), 100) at adv > 2.42:
# two different sets of weights, and the rewards below put adv on both sides of either threshold in every nine rows
# (asserted in tests/test_backward_cases.py)
ALPHA = {0: 0.5, 1: 1.9}
WEIGHT_MODES = (0, 1)
BAR_FLOOR, BAR_FACTOR = FC.BAR_FLOOR, FC.BAR_FACTOR
Case = FC.Case

# ---- the grid --------------------------------------------------------------------------------------------------------
BATCHES, WIDE_BATCHES = (1, 9, 65, 130), (1, 9)
CASES = list(FC.CASES) + [
    # 10 K-tiles of the policy mean; with 17 row tiles (tiles_m >= 16) the slab budget is halved: ktiles 2, 5 slabs
    Case("s60_h580_l1_d6", 60, 6, 580, 1, False, False, 1030, ()),
    # 17 K-tiles of the policy mean: ktiles 2, 9 slabs, the last one leaves mean_skinny_kernel's loop at k0 >= H
    Case("s60_h1028_l1_d2", 60, 2, 1028, 1, False, False, 16, ()),
]
BY_NAME = {c.name: c for c in CASES}
BIG = 1030                          # 17 row tiles: 16 full ones and one of 6 rows

Run = namedtuple("Run", "name B max_batch tune")      # tune: ((key, value), ...) applied to the engine


def _grid():
    runs = []
    for c in FC.CASES:
        for B in (WIDE_BATCHES if c.H >= 2048 else BATCHES):
            if B <= c.max_batch:
                runs.append(Run(c.name, B, c.max_batch, ()))
    runs += [Run("s60_h48_l2_d2", BIG, BIG, ()),
             Run("s60_h48_l2_d2", 130, BIG, (("dw0_slabs", 1),)),
             Run("s60_h48_l2_d2", 130, BIG, (("dw0_slabs", 2),)),
             Run("s60_h580_l1_d6", BIG, BIG, ()),
             Run("s60_h1028_l1_d2", 9, 16, ())]
    return runs


RUNS = _grid()


def run_id(run):
    return f"{run.name}-b{run.B}" + "".join(f"-{k}{v}" for k, v in run.tune)


def max_batch_of(name):
    return max(r.B for r in RUNS if r.name == name)


# ---- the host code's choices (iql_api.inc, skinny.hpp, kernels.hpp), restated ------------------------------------------
SKN_T, SK_MAX = 64, 16
HEAD_ROWS = LN_ROWS_PER_BLOCK = 8
NLL_ROWS_PER_BLOCK = PW_ROWS_PER_BLOCK = 4
NLL_FAST_SLABS = 16
SKINNY_DEFAULT, DW0_SLABS_DEFAULT = 7, 16
SKINNY_PIPELINED_MAX_H = 768
WGRAD, MEAN, OUTBWD = "wgrad_skinny_kernel", "mean_skinny_kernel", "out_bwd_kernel"
SKINNY_KERNELS = (WGRAD, MEAN, OUTBWD)


def cdiv(a, b):
    return -(-a // b)


def skn_split(tiles, max_slabs):
    """-> (nslab, tiles per block)"""
    per = max(1, cdiv(tiles, max_slabs))
    return cdiv(tiles, per), per


def tune_mask(value):
    """porl_tune_set reads the value 1 of a skinny mask as "all"."""
    return 7 if value == 1 else value


def skinny_mask(case, skinny=SKINNY_DEFAULT, short_blocks=False):
    mask = tune_mask(skinny)
    if short_blocks and case.H > SKINNY_PIPELINED_MAX_H:      # skinny_pipelined = -1: by width
        mask = 0
    return mask


def qualifies(case):
    """{kernel: the shape allows it}.  The alignment conditions of the host code hold by construction: every workspace
    buffer and every tensor of an arena starts on 16 bytes, Sp / Hp / Dp are multiples of 4."""
    vec = case.H % 4 == 0
    return {WGRAD: vec and case.S <= SKN_T, MEAN: vec and case.D <= SKN_T, OUTBWD: vec and case.D <= SKN_T}


def skinny_kernels(case, phase, skinny=SKINNY_DEFAULT, short_blocks=False):
    """{kernel: launches} of the skinny kernels in `phase`: "value" (porl_iql_value_backward), "policy" (a
    porl_iql_policy_backward that runs both halves), "forward" (porl_iql_policy_only_forward) or "gradient"
    (porl_iql_policy_backward after a forward half)."""
    mask, ok = skinny_mask(case, skinny, short_blocks), qualifies(case)
    out = {}
    if phase == "value":            # the LayerNorm variant keeps dW0 on the grouped GEMM
        if mask & 1 and ok[WGRAD] and not case.layer_norm:
            out[WGRAD] = 1
        return out
    if phase in ("policy", "forward") and mask & 2 and ok[MEAN]:
        out[MEAN] = 1
    if phase in ("policy", "gradient"):
        if mask & 4 and ok[OUTBWD]:
            out[OUTBWD] = 1
        if mask & 1 and ok[WGRAD]:
            out[WGRAD] = 1
    return out


def splits(case, B, dw0_slabs=DW0_SLABS_DEFAULT):
    """How the three skinny kernels and the per-row kernels walk a batch: (nslab, tiles per block) each, the rows of the
    last slab, the head partials per row and which loop of policy_nll_kernel runs (given the skinny mean)."""
    row_tiles, k_tiles = cdiv(B, SKN_T), cdiv(case.H, SKN_T)
    wgrad = skn_split(row_tiles, dw0_slabs)
    outbwd = skn_split(row_tiles, SK_MAX)
    mean = skn_split(k_tiles, SK_MAX // 2 if row_tiles >= 16 else SK_MAX)
    parts = 1 if case.layer_norm else cdiv(case.H, 32)         # the value twins' head partials (gemm_f32.hpp: head_parts)
    ncl = cdiv(case.D, 64)
    return dict(row_tiles=row_tiles, k_tiles=k_tiles, wgrad=wgrad, outbwd=outbwd, mean=mean, parts=parts, ncl=ncl,
                nll_general=ncl > 1 or mean[0] > NLL_FAST_SLABS or parts > 64,
                head_passes=cdiv(case.H, 1024) if case.H % 4 == 0 else cdiv(case.H, 256))


def short_last_slab(tiles, split):
    """The last slab holds fewer tiles than the others: its block leaves the tile loop by the `b0 >= B` / `k0 >= H` break."""
    nslab, per = split
    return nslab * per > tiles


# ---- parameters and inputs -------------------------------------------------------------------------------------------
NARROW_SCALE = np.float32(2.0 ** -8)
LS_SPECIAL = (-5.0, 2.75, 2.0, -6.5)        # exactly the lower end, above, exactly the upper end, below


def log_std_for(case):
    """(D,) float32.  D >= 4 holds all four special entries at seeded positions and the rest inside (-5, 2); a smaller D
    holds the first D of the list rotated by the case's index, so that the cases with D = 1 and D = 2 cover all four
    between them."""
    i = [c.name for c in CASES].index(case.name)
    rng = np.random.default_rng([77, i])
    ls = rng.uniform(0.2, 1.2, case.D) * rng.choice([-1.0, 1.0], case.D)
    k = min(4, case.D)
    special = [LS_SPECIAL[(i + j) % 4] for j in range(k)] if case.D < 4 else list(LS_SPECIAL)
    ls[rng.permutation(case.D)[:k]] = special
    return np.ascontiguousarray(ls, np.float32)


@lru_cache(maxsize=None)
def params(name):
    """-> (case, arrays as forward_cases.fill with log_std overwritten, oracle state dict)"""
    case = BY_NAME[name]
    arrays = FC.fill(case)
    arrays["log_std"] = log_std_for(case)
    # z = (x - mean) / sigma carries the fp32 error of the mean divided by sigma, 150 times it at sigma = e^-5, and
    # d/dmean = w z / sigma carries it once more into the column that sets the scale of every policy tensor.  At a mean
    # of O(1), whose error after two or three layers is a few 1e-7, two fp32 runs then differ by 1e-5 of scale according to
    # how those few roundings fell (measured: kernel 5 x the numpy run on single tensors, and the reverse).  The output
    # units of the narrow columns are therefore scaled by 2^-8 (exact): their mean is O(1e-2), its error and z's with it.
    for j in np.flatnonzero(arrays["log_std"] <= np.float32(O.LOG_STD_MIN)):
        arrays["policy"]["w"][case.L][j] *= NARROW_SCALE
        arrays["policy"]["b"][case.L][j] *= NARROW_SCALE
    P = FC.oracle_params(case, arrays)
    for v in P.values():
        v.setflags(write=False)
    return case, arrays, P


def _out_act(case):
    return "tanh" if case.pol_tanh else None


def _as(P, dtype):
    return {k: np.asarray(v, dtype) for k, v in P.items()}


def _preacts(P, prefix, x, L, ln):
    """Hidden pre-activations (what ReLU sees) of one MLP in the oracle's current precision."""
    hidden, _ = O.mlp_layer_keys(prefix, L, ln)
    _, cache = O.mlp_forward(P, prefix, x, L, ln)
    out = []
    for i, (lin, lnk) in enumerate(hidden):
        if lnk is not None:
            out.append(cache["xhat"][i] * P[lnk + ".weight"] + P[lnk + ".bias"])
        else:
            out.append(cache["x"][i] @ P[lin + ".weight"].T + P[lin + ".bias"])
    return out


REW_PATTERN = (-3.5, 2.5, -1.0, 0.4, -2.2)      # period 5 against the terminals' period 4


def pool_size(name):
    """About 60 % of random rows are undecided at H ~ 2050 (3 nets x 2 layers x 2050 units, each within MARGIN of zero with
    probability ~ 8e-5), a few per cent at H <= 580: four rows per batch row plus 64 leave the largest batch far inside."""
    return 4 * max_batch_of(name) + 64


@lru_cache(maxsize=None)
def pool(name):
    """The decided rows of case `name`, in pool order: dict(obs, next_obs, rew, term, target, n_pool, n_decided)."""
    case, _, P = params(name)
    n = pool_size(name)
    rng = np.random.default_rng([4242, case.S, case.D, case.H, case.L])
    obs, nxt = rng.standard_normal((n, case.S)), rng.standard_normal((n, case.S))
    for x in (obs, nxt):                       # as forward_cases.inputs: exact zeros and an all-negative column family
        x[:, 1::5] = 0.0
        x[:, 3::5] = -np.abs(x[:, 3::5]) - 0.01
    obs, nxt = np.ascontiguousarray(obs, np.float32), np.ascontiguousarray(nxt, np.float32)
    eps = rng.uniform(0.4, 1.6, (n, case.D)) * rng.choice([-1.0, 1.0], (n, case.D))     # z, in units of sigma
    noise = 0.2 * rng.standard_normal(n)
    O.set_precision(np.float64)
    try:
        P64, x64 = _as(P, np.float64), obs.astype(np.float64)
        ok = np.ones(n, bool)
        for prefix, ln in (("vf.v1", case.layer_norm), ("vf.v2", case.layer_norm), ("goal_policy.net", False)):
            for z in _preacts(P64, prefix, x64, case.L, ln):
                ok &= (np.abs(z) >= MARGIN).all(axis=1)
        mean, _ = O.mlp_forward(P64, "goal_policy.net", x64, case.L, False, _out_act(case))
    finally:
        O.set_precision(np.float32)
    sigma = np.exp(np.clip(P["goal_policy.log_std"].astype(np.float64), O.LOG_STD_MIN, O.LOG_STD_MAX))
    keep = np.flatnonzero(ok)
    k = np.arange(len(keep))
    out = dict(obs=obs[keep], next_obs=nxt[keep],
               rew=np.float32(np.take(REW_PATTERN, k % 5) + noise[keep]), term=np.float32(k % 4 == 2),
               target=np.ascontiguousarray((mean + sigma * eps)[keep], np.float32), n_pool=n, n_decided=len(keep))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def batch(name, B):
    """(obs, next_obs, rew, term, target): the first B decided rows."""
    p = pool(name)
    if p["n_decided"] < B:
        raise ValueError(f"{name}: {p['n_decided']} decided rows of {p['n_pool']} for a batch of {B}")
    return tuple(p[k][:B] for k in ("obs", "next_obs", "rew", "term", "target"))


# ---- the two phases in numpy -------------------------------------------------------------------------------------------
DEFECTS = ("row_dropped", "last_slab_omitted", "wrong_layer_mask", "inside_exclusive", "no_tanh_factor",
           "weight_mode_swapped", "twin_biases_swapped", "term_ignored")


def tensor_names(case, group):
    """Oracle state-dict keys in tensor_table order: group 0 = both online twins, group 1 = log_std + policy net."""
    if group == 0:
        return O.twin_param_names("vf", case.L, case.layer_norm)
    return ["goal_policy.log_std"] + O.mlp_param_names("goal_policy.net", case.L, False)


def _wrong_masks(cache):
    c = dict(cache)
    c["h"] = cache["h"][1:] + cache["h"][:1]          # layer i is gated by layer i + 1's activation
    return c


def _phases(case, P, rows, weight_mode, dtype, defect=None, dw0_slabs=DW0_SLABS_DEFAULT):
    """Both phases on the same un-updated parameters, as the engine runs them without an apply in between.  The policy
    phase weighs with the value phase's target_v and the online twins; policy_weight_kernel forms the same weights from
    the TD target, so the policy-only variant has the same exact-arithmetic answer.  `defect` seeds one of DEFECTS."""
    f = dtype
    L, ln, act = case.L, case.layer_norm, _out_act(case)
    obs, nxt, rew, term, target = (np.asarray(a, f) for a in rows)
    B = obs.shape[0]
    ib = f(1.0) / f(B)
    O.set_precision(dtype)
    try:
        P = _as(P, dtype)
        if defect == "twin_biases_swapped":
            P = dict(P)
            _, last = O.mlp_layer_keys("vf.v1", L, ln)
            k1, k2 = last + ".bias", last.replace("vf.v1", "vf.v2") + ".bias"
            P[k1], P[k2] = P[k2], P[k1]
        if defect == "term_ignored":
            term = np.zeros_like(term)
        k = f(ALPHA[weight_mode])                       # the hyper-parameter stays when the defect swaps the mode
        if defect == "weight_mode_swapped":
            weight_mode = 1 - weight_mode
        # -- value phase (kernels.hpp: relu_head_bwd_kernel / value_loss_kernel) --
        t1, t2, _, _ = O.twin_forward(P, "v_target", nxt, L, ln)
        target_v = rew + (f(1.0) - term) * f(DISCOUNT) * np.minimum(t1, t2)
        v1, v2, c1, c2 = O.twin_forward(P, "vf", obs, L, ln)
        G, us = {}, []
        v_loss = f(0.0)
        for v, c, prefix in ((v1, c1, "vf.v1"), (v2, c2, "vf.v2")):
            u = target_v - v
            w = np.abs(f(TAU) - (u < 0).astype(f))
            v_loss = v_loss + f(0.5) * np.sum(w * u * u, dtype=f) * ib
            dv = -(w * u * ib)
            cc = _wrong_masks(c) if defect == "wrong_layer_mask" else c
            G.update(O.mlp_backward(P, prefix, cc, dv[:, None], L, ln))
            us.append(u)
        # -- policy phase (policy_nll_kernel) --
        adv = target_v - np.minimum(v1, v2)
        raw = np.exp(k * adv if weight_mode else adv / k)
        weight = np.minimum(raw, f(O.EXP_ADV_MAX))
        mean, cp = O.mlp_forward(P, "goal_policy.net", obs, L, False, act)
        log_std = P["goal_policy.log_std"]
        nlp, z, sigma = O.gaussian_nll(mean, target, log_std)
        d_mean, d_ls = O.policy_nll_grads(z, sigma, log_std, weight * ib)
        if defect == "inside_exclusive":
            d_ls = d_ls * ((log_std > f(O.LOG_STD_MIN)) & (log_std < f(O.LOG_STD_MAX)))
        cc = _wrong_masks(cp) if defect == "wrong_layer_mask" else cp
        G.update(O.mlp_backward(P, "goal_policy.net", cc, d_mean, L, False, None if defect == "no_tanh_factor" else act))
        G["goal_policy.log_std"] = d_ls
        stats = np.array([v_loss, np.sum(weight * nlp, dtype=f) * ib, nlp.min()], dtype=f)
        if defect in ("row_dropped", "last_slab_omitted"):
            # a weight gradient is a sum over batch rows: the same phases on fewer rows (same 1 / B) give the sum without them
            if defect == "row_dropped":
                keep, names = B - 1, ["vf.v2.0.weight", "goal_policy.net.0.weight"]
            else:                                          # rows of the last slab of wgrad_skinny_kernel / out_bwd_kernel
                nslab, per = skn_split(cdiv(B, SKN_T), dw0_slabs)
                keep = (nslab - 1) * per * SKN_T
                _, last = O.mlp_layer_keys("goal_policy.net", L, False)
                names = ["vf.v1.0.weight", last + ".weight"]
            short = _phases_scaled(case, P, tuple(a[:keep] for a in rows), weight_mode, dtype, B)
            for n in names:
                G[n] = short[n]
    finally:
        O.set_precision(np.float32)
    return dict(grads=G, stats=stats, u=us, raw_weight=raw, weight=weight, target_v=target_v, nlp=nlp)


def _phases_scaled(case, P, rows, weight_mode, dtype, B_full):
    """Gradients of `rows` scaled by 1 / B_full (zeros when no row is left)."""
    if rows[0].shape[0] == 0:
        return {k: np.zeros_like(np.asarray(v, dtype)) for k, v in P.items()}
    G = _phases(case, P, rows, weight_mode, dtype)["grads"]
    s = dtype(rows[0].shape[0]) / dtype(B_full)
    return {k: v * s for k, v in G.items()}


def losses64(name, B, weight_mode, P64):
    """(v_loss, g_loss) in fp64 as functions of the parameters `P64`, the policy loss with the weights held at their
    value under the case's own parameters (the reference detaches them): what finite differences are taken of."""
    case = BY_NAME[name]
    weight = backward64(name, B, weight_mode)["weight"]
    obs, nxt, rew, term, target = (np.asarray(a, np.float64) for a in batch(name, B))
    O.set_precision(np.float64)
    try:
        t1, t2, _, _ = O.twin_forward(P64, "v_target", nxt, case.L, case.layer_norm)
        target_v = rew + (1.0 - term) * DISCOUNT * np.minimum(t1, t2)
        v1, v2, _, _ = O.twin_forward(P64, "vf", obs, case.L, case.layer_norm)
        v_loss = sum(0.5 * O.asymmetric_l2(target_v - v, TAU)[0] for v in (v1, v2))
        mean, _ = O.mlp_forward(P64, "goal_policy.net", obs, case.L, False, _out_act(case))
        nlp, _, _ = O.gaussian_nll(mean, target, P64["goal_policy.log_std"])
        return float(v_loss), float(np.mean(weight * nlp))
    finally:
        O.set_precision(np.float32)


@lru_cache(maxsize=None)
def backward64(name, B, weight_mode):
    case, _, P = params(name)
    out = _phases(case, P, batch(name, B), weight_mode, np.float64)
    for g in out["grads"].values():
        g.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def backward32(name, B, weight_mode):
    case, _, P = params(name)
    return _phases(case, P, batch(name, B), weight_mode, np.float32)


def defective32(name, B, weight_mode, defect, dw0_slabs=DW0_SLABS_DEFAULT):
    case, _, P = params(name)
    return _phases(case, P, batch(name, B), weight_mode, np.float32, defect, dw0_slabs)


def tensor_error(got, ref64):
    """max |got - ref64| / max |ref64| over the tensor; an all-zero reference allows nothing but zeros (error 0 or inf)."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    scale = float(np.abs(ref64).max())
    if scale == 0.0:
        return 0.0 if not got.any() else float("inf")
    return float(np.abs(got - ref64).max() / scale)


def errors(case, got, ref64):
    """{tensor name or "stats<i>": error} of a result dict(grads=, stats=) against the fp64 one."""
    out = {n: tensor_error(got["grads"][n], ref64["grads"][n]) for g in (0, 1) for n in tensor_names(case, g)}
    out.update({f"stats{i}": tensor_error(got["stats"][i], ref64["stats"][i]) for i in range(3)})   # each on its own scale
    return out


@lru_cache(maxsize=None)
def reference(name, B, weight_mode):
    """-> dict(ref = the fp64 result, e32 = {output: error of the fp32 run}, bar = {output: limit}), computed once and shared.
    The policy-only variant (weights from the TD target, policy_weight_kernel) has the same reference for group 1 and
    stats[1:3]: with no apply between the phases it weighs with the same target_v and the same twins."""
    case = BY_NAME[name]
    ref = backward64(name, B, weight_mode)
    e32 = errors(case, backward32(name, B, weight_mode), ref)
    return dict(ref=ref, e32=e32, bar={k: max(BAR_FLOOR, BAR_FACTOR * e) for k, e in e32.items()})


def clamped_out(name):
    """Indices of log_std outside [-5, 2]: d/dlog_std is exactly zero there."""
    ls = params(name)[2]["goal_policy.log_std"]
    return np.flatnonzero((ls < O.LOG_STD_MIN) | (ls > O.LOG_STD_MAX))
