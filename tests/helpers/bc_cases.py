"""Cases of the goal-conditioned behaviour-cloning step (porl_iql_load_batch_cat / _pairs, porl_iql_bc_forward /
porl_iql_bc_step; reference agent/por.py:178-184): tests/test_goal_bc_cases.py checks them on the CPU,
tests/test_goal_bc_gpu.py runs them on the device.  numpy only, no device use.

The step is restated from oracle.por_oracle's pieces — mlp_forward, gaussian_nll, policy_nll_grads (unit weights),
mlp_backward, adam_step, cosine_lr — at fp64 (the yardstick) and at fp32 (whose error against fp64 sets the bar).

Inputs, built as tests/helpers/backward_cases.py builds them.  A configuration has a packed-row store
[s | r | s' | d | a]; sample i is (start row, goal row): the policy's input is [s of start | columns goal_col.. of goal]
and its regression target the action columns of start.  goal_col = S + 1 reads the start row's own s' (POR's [s | s']),
goal_col = 0 the state of another row (a hindsight goal).  The only discontinuities of the step are the policy net's
ReLU gates: a store row is DECIDED when, in fp64, every hidden pre-activation of its sample has |z| >= MARGIN, and a batch
is the first B decided rows, so no row is ever left out of a comparison.  log_std carries entries on, inside and
outside [-5, 2] (`log_std_for`); the stored actions are the fp64 policy mean plus a multiple of sigma per column, |z| in
[0.4, 1.6]; the output units of the columns with sigma = e^-5 are scaled by 2^-8 (backward_cases.params says why).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from helpers import backward_cases as BC
from helpers import forward_cases as FC
from oracle import por_oracle as O

MARGIN = BC.MARGIN
BAR_FLOOR, BAR_FACTOR = FC.BAR_FLOOR, FC.BAR_FACTOR
PREFIX = "policy"                      # state-dict prefix of GoalConditionedBC.policy
LR0, T_MAX = 1e-4, 1000                # policy_lr, max_steps of the one-step check

Config = namedtuple("Config", "name S G goal_col A H L tanh")

CONFIGS = [
    Config("s60_g60_c61_a2_h48_l2", 60, 60, 61, 2, 48, 2, False),         # POR's [s | s'], the plain shape
    Config("s60_g2_c0_a2_h132_l2_tanh", 60, 2, 0, 2, 132, 2, True),       # position goal of a later row; S + G = 62: Sp = 64
    Config("s3_g1_c4_a1_h30_l1_tanh", 3, 1, 4, 1, 30, 1, True),           # no 16-byte lane in a row; H % 4 != 0; L = 1
    Config("s17_g17_c0_a6_h48_l3", 17, 17, 0, 6, 48, 3, False),           # a scalar tail after four 16-byte lanes; A = 6: all four special log_std entries
    Config("s182_g182_c183_a2_h48_l2", 182, 182, 183, 2, 48, 2, False),   # input width 364 > 256: no l0 / skinny dW0 kernel
]
BY_NAME = {c.name: c for c in CONFIGS}
BATCHES = (1, 9, 65, 130)
BIG = 1030                             # 17 row tiles, first configuration only
RUNS = [(c.name, B) for c in CONFIGS for B in BATCHES] + [(CONFIGS[0].name, BIG)]


def max_batch_of(name):
    return max(B for n, B in RUNS if n == name)


def engine_case(cfg):
    """The configuration as a forward_cases.Case of the engine: obs_dim = S + G, pol_out_dim = A."""
    return FC.Case(cfg.name, cfg.S + cfg.G, cfg.A, cfg.H, cfg.L, False, cfg.tanh, max_batch_of(cfg.name), ())


def row_width(cfg):
    return 2 * cfg.S + 2 + cfg.A


def log_std_for(cfg):
    """(A,) float32 in the manner of backward_cases.log_std_for: A >= 4 holds all four special entries (exactly -5, above
    2, exactly 2, below -5) and the rest inside; a smaller A the first A of the list rotated by the configuration's index,
    so that the configurations with A = 1 and A = 2 cover all four between them."""
    i = [c.name for c in CONFIGS].index(cfg.name)
    rng = np.random.default_rng([78, i])
    ls = rng.uniform(0.2, 1.2, cfg.A) * rng.choice([-1.0, 1.0], cfg.A)
    k = min(4, cfg.A)
    special = [BC.LS_SPECIAL[(i + j) % 4] for j in range(k)] if cfg.A < 4 else list(BC.LS_SPECIAL)
    ls[rng.permutation(cfg.A)[:k]] = special
    return np.ascontiguousarray(ls, np.float32)


def param_names(cfg):
    """State-dict keys in the engine's tensor_table order of group 1: log_std first, then the net."""
    return [PREFIX + ".log_std"] + O.mlp_param_names(PREFIX + ".net", cfg.L, False)


@lru_cache(maxsize=None)
def params(name):
    """-> (cfg, {state-dict key: float32 array}), read-only."""
    cfg = BY_NAME[name]
    case = engine_case(cfg)
    net = FC.fill(case)["policy"]
    ls = log_std_for(cfg)
    for j in np.flatnonzero(ls <= np.float32(O.LOG_STD_MIN)):
        net["w"][cfg.L][j] *= BC.NARROW_SCALE
        net["b"][cfg.L][j] *= BC.NARROW_SCALE
    tensors = [ls]
    for l in range(cfg.L + 1):
        tensors += [net["w"][l], net["b"][l]]
    P = dict(zip(param_names(cfg), tensors))
    for v in P.values():
        v.setflags(write=False)
    return cfg, P


def _out_act(cfg):
    return "tanh" if cfg.tanh else None


def _as(P, dtype):
    return {k: np.asarray(v, dtype) for k, v in P.items()}


def pool_size(name):
    """Four store rows per batch row plus 64: a few per cent of random rows are undecided at these widths."""
    return 4 * max_batch_of(name) + 64


def goal_rows(cfg, n):
    """The goal row of every store row: the row itself where the goal is its own s', else another row of the store
    (row 0's partner is row 3, every seventh row is its own goal: goal == start occurs)."""
    i = np.arange(n, dtype=np.int64)
    if cfg.goal_col == cfg.S + 1:
        return i
    g = (i * 5 + 3) % n
    g[::7] = i[::7]
    return g


def gather_inputs(cfg, rows, start, goal):
    """[s of start | goal columns of goal] and the action columns of start — what the loaders stage."""
    S, G, c = cfg.S, cfg.G, cfg.goal_col
    x = np.concatenate([rows[start, :S], rows[goal, c:c + G]], axis=1)
    return np.ascontiguousarray(x), np.ascontiguousarray(rows[start, 2 * S + 2:2 * S + 2 + cfg.A])


@lru_cache(maxsize=None)
def pool(name):
    """dict(rows = the (n, 2S+2+A) float32 store, goal = (n,) goal row of every row, decided = the decided rows in store
    order, n_pool, n_decided).  Rewards are 7.0 and the flags follow a period of 4: a loader that reads a neighbouring
    column stages a number no state holds."""
    cfg, P = params(name)
    n = pool_size(name)
    S, G, A = cfg.S, cfg.G, cfg.A
    rng = np.random.default_rng([4343, S, G, A, cfg.H, cfg.L])
    rows = np.zeros((n, row_width(cfg)), np.float32)
    for lo in (0, S + 1):                      # s and s', as forward_cases.inputs: exact zeros, an all-negative column family
        x = rng.standard_normal((n, S))
        x[:, 1::5] = 0.0
        x[:, 3::5] = -np.abs(x[:, 3::5]) - 0.01
        rows[:, lo:lo + S] = x
    rows[:, S] = 7.0
    rows[:, 2 * S + 1] = np.arange(n) % 4 == 2
    goal = goal_rows(cfg, n)
    eps = rng.uniform(0.4, 1.6, (n, A)) * rng.choice([-1.0, 1.0], (n, A))       # z, in units of sigma
    x, _ = gather_inputs(cfg, rows, np.arange(n), goal)
    O.set_precision(np.float64)
    try:
        P64, x64 = _as(P, np.float64), x.astype(np.float64)
        ok = np.ones(n, bool)
        for z in BC._preacts(P64, PREFIX + ".net", x64, cfg.L, False):
            ok &= (np.abs(z) >= MARGIN).all(axis=1)
        mean, _ = O.mlp_forward(P64, PREFIX + ".net", x64, cfg.L, False, _out_act(cfg))
    finally:
        O.set_precision(np.float32)
    sigma = np.exp(np.clip(P[PREFIX + ".log_std"].astype(np.float64), O.LOG_STD_MIN, O.LOG_STD_MAX))
    rows[:, 2 * S + 2:] = mean + sigma * eps
    out = dict(rows=rows, goal=goal, decided=np.flatnonzero(ok), n_pool=n, n_decided=int(ok.sum()))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def pairs(name, B):
    """(start, goal): the first B decided rows and their goal rows, int64."""
    p = pool(name)
    if p["n_decided"] < B:
        raise ValueError(f"{name}: {p['n_decided']} decided rows of {p['n_pool']} for a batch of {B}")
    start = p["decided"][:B].astype(np.int64)
    return start, p["goal"][start]


def batch(name, B):
    """(x, actions): the policy's input and regression target for `pairs(name, B)`."""
    cfg = BY_NAME[name]
    return gather_inputs(cfg, pool(name)["rows"], *pairs(name, B))


# ---- the step in numpy -------------------------------------------------------------------------------------------------
def bc_grads(cfg, P, x, actions, dtype):
    """por.py:178-180 and its backward at working precision `dtype` -> dict(grads = {key: array}, stats = [loss, min NLL]).
    P is not modified."""
    f = dtype
    O.set_precision(dtype)
    try:
        P = _as(P, dtype)
        x, actions = np.asarray(x, f), np.asarray(actions, f)
        B = x.shape[0]
        ib = f(1.0) / f(B)
        mean, cache = O.mlp_forward(P, PREFIX + ".net", x, cfg.L, False, _out_act(cfg))
        log_std = P[PREFIX + ".log_std"]
        nlp, z, sigma = O.gaussian_nll(mean, actions, log_std)
        d_mean, d_ls = O.policy_nll_grads(z, sigma, log_std, np.full(B, ib, f))            # unit weights over B
        G = O.mlp_backward(P, PREFIX + ".net", cache, d_mean, cfg.L, False, _out_act(cfg))
        G[PREFIX + ".log_std"] = d_ls
        stats = np.array([np.sum(nlp, dtype=f) * ib, nlp.min()], dtype=f)
    finally:
        O.set_precision(np.float32)
    return dict(grads=G, stats=stats)


class BcOracle:
    """K steps of por.py:178-184: the gradients above, torch's Adam (oracle adam_step) at the cosine schedule's rate for
    this step (oracle cosine_lr), then the schedule moves."""

    def __init__(self, cfg, P, dtype, lr0=LR0, t_max=T_MAX):
        self.cfg, self.dtype, self.lr0, self.t_max = cfg, dtype, lr0, t_max
        self.P = {k: np.array(v, dtype=dtype, copy=True) for k, v in P.items()}
        self.adam = O.AdamState(lr0, param_names(cfg))
        self.t = 0
        self.last_min_nll = float("nan")

    def update(self, x, actions):
        out = bc_grads(self.cfg, self.P, x, actions, self.dtype)
        O.set_precision(self.dtype)
        try:
            O.adam_step(self.P, out["grads"], self.adam, lr=O.cosine_lr(self.lr0, self.t, self.t_max))
        finally:
            O.set_precision(np.float32)
        self.t += 1
        self.last_min_nll = float(out["stats"][1])
        return float(out["stats"][0])


@lru_cache(maxsize=None)
def reference(name, B):
    """-> dict(ref = the fp64 gradients and statistics, e32 / bar = {key or "stats<i>": fp32 error / limit}, params64 = the
    fp64 parameters after ONE step), computed once and shared, read-only.  The error of a tensor is
    max |got - ref64| / max |ref64| (backward_cases.tensor_error), its bar max(BAR_FLOOR, BAR_FACTOR x e32)."""
    cfg, P = params(name)
    x, a = batch(name, B)
    ref = bc_grads(cfg, P, x, a, np.float64)
    got32 = bc_grads(cfg, P, x, a, np.float32)
    e32 = errors(cfg, got32, ref)
    o = BcOracle(cfg, P, np.float64)
    o.update(x, a)
    for g in list(ref["grads"].values()) + list(o.P.values()):
        g.setflags(write=False)
    return dict(ref=ref, e32=e32, bar={k: max(BAR_FLOOR, BAR_FACTOR * e) for k, e in e32.items()}, params64=o.P)


def errors(cfg, got, ref64):
    out = {n: BC.tensor_error(got["grads"][n], ref64["grads"][n]) for n in param_names(cfg)}
    out.update({f"stats{i + 1}": BC.tensor_error(got["stats"][i], ref64["stats"][i]) for i in range(2)})
    return out


def clamped_out(name):
    """Indices of log_std outside [-5, 2]: d/dlog_std is exactly zero there."""
    ls = params(name)[1][PREFIX + ".log_std"]
    return np.flatnonzero((ls < O.LOG_STD_MIN) | (ls > O.LOG_STD_MAX))
