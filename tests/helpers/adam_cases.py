"""Seeded cases of the Adam / Polyak sweep (csrc/kernels.hpp: adam_ema_kernel, ema_kernel; csrc/porl_api.hip: adam_launch),
shared by the CPU checks (tests/test_adam_cases.py) and the GPU comparisons (tests/test_adam_sweep_gpu.py,
tests/test_adam_fold_gpu.py): the update in fp64 (`adam64` of qstep_cases, `ema64`: the yardstick), in fp32 operation for
operation (`adam32`, `ema32`: the control), the bars, the table of sweep calls and the cases of the folded launch.
numpy only.

    m' = m + (1 - b1) (g - m),   v' = b2 v + (1 - b2) g^2,   p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    t' = (1 - beta) t + beta p'                                             (Polyak, on the NEW parameters)

The bars are the project's own, stated before these tests existed and not tuned against the kernels: parameters, m and v
from tests/test_qstep_gpu.py, the target from tests/test_gemm_gpu.py.  They hold for moments "of a run in progress", drawn as
qstep_cases.make draws them (|m| <~ 2e-3, sqrt(v) >= 5e-3): where m + (1 - b1)(g - m) cancels, fp32 leaves about half an
ulp of each term, which the 1e-9 absolute bar on m has to take."""
import math
import zlib

import numpy as np

from helpers.qstep_cases import adam64            # the fp64 yardstick: reused, not copied

f32 = np.float32
EPS = 1e-8
# quantity: (atol, rtol)
BARS = {"p": (1e-7, 1e-6), "m": (1e-9, 1e-5), "v": (1e-12, 1e-5), "t": (1e-7, 1e-6)}

# Hyper-parameters of the folded cases and of the mutated controls, chosen so that every defect of MUTATIONS (and of the
# hand mutations recorded in tests/test_adam_fold_gpu.py) moves its quantity by at least 100 bars.  With moments of a run
# in progress the step is lr * r, r = m^ / sqrt(v^) ~ 0.1 .. 0.5 once the bias corrections are of order one (at t = 7 they
# would shrink r by six: sqrt(1 - b2^7) = 0.084), so the steps are those of a run in progress too.  A Polyak line left out
# then lags a target by beta |p' - t| ~ 0.05 * 0.3, one that reads the old parameters by beta * lr * r ~ 1e-4, against a
# bar of at most 6e-7; sqrt(1 - b2^t) is 0.71 at t = 700 and 0.51 at t = 300, far from its square.
LR, EMA_BETA, BETAS = 1e-2, 0.05, (0.9, 0.999)
VALUE_STEP, POLICY_STEP = 700, 300
HOST_G = 5e-2                                     # gradient scale of the host cases
P_MAX = 0.5                                       # |p|, |t| <= P_MAX


# ---- the update ---------------------------------------------------------------------------------------------------------
def scalars(lr, step, betas=BETAS, eps=EPS, ema_beta=0.0):
    """adam_launch's host scalars: python doubles, rounded to fp32 where they meet tensors."""
    b1, b2 = betas
    return dict(step_size=f32(lr / (1.0 - b1 ** step)), bc2_sqrt=f32(math.sqrt(1.0 - b2 ** step)), omb1=f32(1.0 - b1),
                beta2=f32(b2), omb2=f32(1.0 - b2), eps=f32(eps), ema_beta=f32(ema_beta), omeb=f32(1.0 - ema_beta))


def fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double
    rounding that differs from fmaf in about one case in 2^29: immaterial to a control that is compared at bars)."""
    return (np.asarray(a, dtype=f32).astype(np.float64) * np.asarray(b, dtype=f32).astype(np.float64)
            + np.asarray(c, dtype=f32).astype(np.float64)).astype(f32)


def adam32(p, g, m, v, lr, step, betas=BETAS, eps=EPS, s=None):
    """adam1 of csrc/kernels.hpp, operation for operation in fp32 -> (p, m, v).  `s`: scalars to use instead (mutations)."""
    s = s or scalars(lr, step, betas, eps)
    p, g, m, v = (np.asarray(x, dtype=f32) for x in (p, g, m, v))
    with np.errstate(under="ignore", over="ignore"):
        m = fma32(s["omb1"], g - m, m)
        v = fma32(s["omb2"] * g, g, v * s["beta2"])
        p = fma32(-s["step_size"], m / (np.sqrt(v) / s["bc2_sqrt"] + s["eps"]), p)
    return p, m, v


def ema32(t, p_new, ema_beta):
    """ema1 of csrc/kernels.hpp in fp32."""
    t, p_new = np.asarray(t, dtype=f32), np.asarray(p_new, dtype=f32)
    return fma32(f32(ema_beta), p_new, t * f32(1.0 - ema_beta))


def ema64(t, p_new, ema_beta):
    """t (1 - beta) + beta p' in fp64, beta and 1 - beta rounded to fp32 first, as adam_launch rounds them."""
    b, omb = float(f32(ema_beta)), float(f32(1.0 - ema_beta))
    return np.asarray(t, dtype=np.float64) * omb + b * np.asarray(p_new, dtype=np.float64)


def oracle(d):
    """fp64 result of one call `d` (see `draw`): dict p, m, v and t (None without a target)."""
    p, m, v = adam64(d["p"], d["g"], d["m"], d["v"], lr=d["lr"], step=d["step"], betas=d["betas"], eps=EPS)
    return dict(p=p, m=m, v=v, t=None if d["t"] is None else ema64(d["t"], p, d["ema_beta"]))


def control(d, s=None):
    """The fp32 control of the same call."""
    p, m, v = adam32(d["p"], d["g"], d["m"], d["v"], d["lr"], d["step"], d["betas"], EPS, s=s)
    return dict(p=p, m=m, v=v, t=None if d["t"] is None else ema32(d["t"], p, d["ema_beta"]))


def excess(got, want, q):
    """Largest |got - want| / (atol + rtol |want|) of quantity q: <= 1 is inside the bar."""
    atol, rtol = BARS[q]
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float((err / (atol + rtol * np.abs(want))).max()) if err.size else 0.0


def excesses(got, want):
    return {q: excess(got[q], want[q], q) for q in BARS if want.get(q) is not None}


# ---- inputs -------------------------------------------------------------------------------------------------------------
G_KINDS = ("normal", "zero", "big", "tiny_v0", "underflow", "mixed")


def moments(rng, n):
    """Moments of a run in progress, drawn exactly as qstep_cases.make draws them."""
    m = (5e-4 * rng.standard_normal(n)).astype(f32)
    v = ((0.01 * (0.5 + np.abs(rng.standard_normal(n)))) ** 2).astype(f32)
    return m, v


def gradient(rng, n, kind, scale=1e-2):
    """-> (g, fresh): `fresh` marks the elements whose moments start at zero (the eps-dominated denominator)."""
    col = {"normal": 0, "zero": 1, "big": 2, "tiny_v0": 3, "underflow": 4}
    k = np.arange(n) % 5 if kind == "mixed" else np.full(n, col[kind])
    sign = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    g = np.select([k == 0, k == 1, k == 2, k == 3, k == 4],
                  [scale * rng.standard_normal(n), 0.0, 1e3 * (0.5 + rng.uniform(size=n)) * sign,
                   1e-12 * (0.5 + rng.uniform(size=n)) * sign, 1e-22 * sign])
    return g.astype(f32), k == 3


def draw(name, n, lr, step, betas=BETAS, ema_beta=None, gkind="normal", gscale=1e-2):
    """One call of the sweep on n elements: p, g, m, v, t (None when ema_beta is None) as fp32 arrays, seeded by name."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    p = rng.uniform(-P_MAX, P_MAX, n).astype(f32)
    t = None if ema_beta is None else rng.uniform(-P_MAX, P_MAX, n).astype(f32)
    m, v = moments(rng, n)
    g, fresh = gradient(rng, n, gkind, gscale)
    m[fresh], v[fresh] = 0.0, 0.0
    return dict(name=name, n=n, lr=lr, step=step, betas=betas, ema_beta=ema_beta, gkind=gkind, p=p, g=g, m=m, v=v, t=t)


# ---- the table of sweep calls (tests/test_adam_sweep_gpu.py) ------------------------------------------------------------
# Sizes on either side of a 256-float4 block (1024 floats) and of a block count; the largest occurs once.
SIZES = (4, 8, 1020, 1024, 1028, 3076, 65540, 1048588)
STEPS = (1, 2, 10, 1000, 100000)
LRS = (0.0, 3e-4, 1e-2)
BETA_PAIRS = ((0.9, 0.999), (0.5, 0.9))
EMA_BETAS = (None, 0.0, 0.005, 0.05, 1.0)        # None: no target
OFFSETS = (4, 8, 12, 64, 1024)                   # where the call's slice starts in the longer buffer (floats, multiples of 4)


def _table():
    """Not the product of the axes: 36 rows in which every value of every axis occurs (tests/test_adam_cases.py checks it).
    Row i walks each axis at its own stride, so the pairings vary."""
    rows = []
    for i in range(35):
        rows.append(dict(n=SIZES[i % 7], step=STEPS[i % 5], lr=LRS[(i + i // 3) % 3], betas=BETA_PAIRS[(i + i // 2) % 2],
                         ema_beta=EMA_BETAS[(i + i // 5) % 5], gkind=G_KINDS[(i + i // 6) % 6], off=OFFSETS[(i + i // 7) % 5]))
    rows.append(dict(n=SIZES[7], step=10, lr=1e-2, betas=BETA_PAIRS[0], ema_beta=0.005, gkind="mixed", off=8))
    for r in rows:
        e = "none" if r["ema_beta"] is None else f"{r['ema_beta']:g}"
        r["name"] = f"n{r['n']}-t{r['step']}-lr{r['lr']:g}-b{r['betas'][0]:g}-ema{e}-{r['gkind']}-o{r['off']}"
    return rows


TABLE = _table()
TABLE_BY_NAME = {r["name"]: r for r in TABLE}
assert len(TABLE_BY_NAME) == len(TABLE)


def draw_row(row):
    return draw(row["name"], row["n"], row["lr"], row["step"], row["betas"], row["ema_beta"], row["gkind"])


# ---- the mutated controls -----------------------------------------------------------------------------------------------
# Calls at the hyper-parameters of the folded cases; [lo, hi) is the sub-range a reduce+Adam block would own.
# name: (n, step, target, lo, hi)
HOST_CASES = {
    "value-bias": (4104, VALUE_STEP, True, 4100, 4101),        # one output-bias element, as v.b[L]
    "value-head": (4104, VALUE_STEP, True, 2048, 2112),        # a 64-wide head weight
    "value-ragged": (1028, VALUE_STEP, True, 100, 950),        # a (50, 17) dW0
    "policy-logstd": (1028, POLICY_STEP, False, 0, 17),
    "policy-head": (65540, POLICY_STEP, False, 65000, 65540),
}


def draw_host(name):
    n, step, target, lo, hi = HOST_CASES[name]
    d = draw("host-" + name, n, LR, step, BETAS, EMA_BETA if target else None, "normal", HOST_G)
    d["lo"], d["hi"] = lo, hi
    return d


def _no_polyak(d):
    r = control(d)
    r["t"][d["lo"]:d["hi"]] = d["t"][d["lo"]:d["hi"]]
    return r


def _polyak_from_old(d):
    r = control(d)
    sl = slice(d["lo"], d["hi"])
    r["t"][sl] = ema32(d["t"][sl], d["p"][sl], d["ema_beta"])
    return r


def _stepped_twice(d):
    r = control(d)
    sl = slice(d["lo"], d["hi"])
    p, m, v = adam32(r["p"][sl], d["g"][sl], r["m"][sl], r["v"][sl], d["lr"], d["step"], d["betas"])
    r["p"][sl], r["m"][sl], r["v"][sl] = p, m, v
    if r["t"] is not None:
        r["t"][sl] = ema32(r["t"][sl], p, d["ema_beta"])
    return r


def _bc2_no_sqrt(d):
    s = scalars(d["lr"], d["step"], d["betas"])
    s["bc2_sqrt"] = f32(1.0 - d["betas"][1] ** d["step"])
    return control(d, s)


def _beta2_swapped(d):
    s = scalars(d["lr"], d["step"], d["betas"])
    s["beta2"], s["omb2"] = s["omb2"], s["beta2"]
    return control(d, s)


# name: (mutated control, needs a target, the quantities it must push outside their bars)
MUTATIONS = {
    "no_polyak_on_subrange": (_no_polyak, True, ("t",)),
    "polyak_from_p_old": (_polyak_from_old, True, ("t",)),
    "element_stepped_twice": (_stepped_twice, False, ("p", "m", "v")),
    "bc2_without_sqrt": (_bc2_no_sqrt, False, ("p",)),
    "beta2_for_one_minus_beta2": (_beta2_swapped, False, ("p", "v")),
}
SHARP = 100.0                                     # a mutation must exceed a bar by this factor


# ---- the folded launch (tests/test_adam_fold_gpu.py) ---------------------------------------------------------------------
PLAN = ("regions", "fold32", "fold4", "unfolded", "skips", "reduce_blocks")       # IqlEngine.ADAM_PLAN
# Derived from HEAD_ROWS = 8 (head partials: ceil(B / 8)), NLL_ROWS_PER_BLOCK = 4 (NLL partials: ceil(B / 4)), skn_split
# (ceil(B / 64) batch tiles over at most 16 slabs), pick_splitk (at most K / 64 slabs of a grouped GEMM: none below a batch
# of 128), ADAM_SWEEP_SLABS = 16 and add_reduce's width (4 beyond 64 slabs).  A job is a region when its output and slab
# stride are multiples of 4 floats and it has at most 16 slabs; otherwise reduce+Adam blocks of 32 (or 4) outputs each.
# Three batches differ from the issue's table, for the reason given there: pick_splitk splits the batch dimension of a
# grouped-GEMM dW0 only from K / 64 >= 2, so the cases whose dW0 goes through the grouped GEMM need B >= 128 to leave a
# combine behind at all (ln: 50 -> 150, s70: 64 -> 128, h50: 40 -> 128).
# name: S, H, L, B, layer_norm, D, plan of the value group, plan of the policy group, what it exercises
FOLD_CASES = {
    "d17": (17, 48, 2, 32, False, 17, (6, 2, 0, 1, 2, 3), (3, 2, 0, 2, 2, 4),
            "4 head slabs and one dW0 slab as regions; the D = 17 log_std and output-bias jobs as width-32 blocks with "
            "ragged skip ranges"),
    "slabs16": (60, 64, 2, 128, False, 60, (6, 2, 0, 1, 2, 3), (4, 1, 0, 2, 1, 4),
                "16 head slabs, the last count that is a region; log_std at 32 slabs, width 32"),
    "slabs17": (60, 64, 2, 136, False, 60, (4, 4, 0, 1, 4, 7), (4, 1, 0, 2, 1, 4),
                "17 head slabs leave the sweep for width 32; 3 dW0 slabs, the last batch chunk ragged"),
    "width4": (60, 64, 1, 520, False, 60, (4, 0, 4, 1, 4, 35), (4, 0, 1, 2, 1, 17),
               "65 head partials and 130 NLL partials, both width 4; one hidden layer"),
    "ln": (20, 100, 2, 150, True, 20, (4, 0, 0, 0, 0, 0), (4, 1, 0, 2, 1, 3),
           "LayerNorm: only the dW0 combine (2 split-K slabs of the grouped GEMM) is deferred"),
    "tiles18": (8, 132, 3, 1100, False, 8, (4, 0, 4, 1, 4, 69), (4, 0, 1, 2, 1, 4),
                "18 batch tiles give 9 dW0 slabs; three column tiles; three hidden layers"),
    "s70": (70, 64, 2, 128, False, 70, (6, 2, 0, 1, 2, 3), (3, 2, 0, 2, 2, 8),
            "S > 64: the skinny kernels decline, the grouped GEMM's split-K slabs feed the regions"),
    "h50": (17, 50, 2, 128, False, 17, (0, 8, 0, 1, 8, 65), (0, 5, 0, 2, 5, 60),
            "H % 4 != 0: nothing is a region, dW0 itself goes through ragged reduce+Adam blocks"),
    "act4": (60, 64, 2, 136, False, 4, (4, 4, 0, 1, 4, 7), (4, 1, 0, 2, 1, 3),
             "action-target form: D = 4 with a (B, 4) policy target"),
}


def fold_state(name, tables, sizes):
    """Seeded state of a fold case.  tables: {group: [(offset, shape)]}; sizes: {group: floats of the flat buffer}.
    -> {group: dict(p, t, m, v)} flat fp32 arrays, zero outside the tensors; 2-D tensors ~ N(0, 1 / fan_in), 1-D uniform,
    everything within +-P_MAX; the target a draw of its own; moments of a run in progress."""
    rng = np.random.default_rng(zlib.crc32(("fold-" + name).encode()))
    out = {}
    for g in sorted(tables):
        flat = {k: np.zeros(sizes[g], dtype=f32) for k in ("p", "t", "m", "v")}
        for off, shape in tables[g]:
            n = int(np.prod(shape))
            for k in ("p", "t"):
                x = rng.standard_normal(n) / math.sqrt(shape[-1]) if len(shape) == 2 else rng.uniform(-0.3, 0.3, n)
                flat[k][off:off + n] = np.clip(x, -P_MAX, P_MAX).astype(f32)
            flat["m"][off:off + n], flat["v"][off:off + n] = moments(rng, n)
        out[g] = flat
    return out


def fold_batch(name, S, D, B):
    rng = np.random.default_rng(zlib.crc32(("batch-" + name).encode()))
    return dict(obs=rng.standard_normal((B, S)).astype(f32), next_obs=rng.standard_normal((B, S)).astype(f32),
                rew=rng.standard_normal(B).astype(f32), term=(rng.uniform(size=B) < 0.25).astype(f32),
                pol_target=rng.standard_normal((B, D)).astype(f32))
