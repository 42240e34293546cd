"""The exported sweeps on their own, per element: porl_adam_ema against adam64 / ema64 over the table of
tests/helpers/adam_cases.py (sizes on either side of a 256-float4 block and of a block count, steps 1 .. 100000, lr 0 ..
1e-2, two beta pairs, no target and ema_beta 0 .. 1, gradients normal / zero / ~1e3 / ~1e-12 on fresh moments / 1e-22),
each call on a slice of a longer buffer whose sentinels on both sides must come back bit-unchanged in all five arrays, as
must g; porl_ema against ema64 and bit for bit against the target the fused sweep leaves for the same parameters;
porl_reduce_mean bit for bit on exactly summable inputs.

The bars are the project's own (helpers/adam_cases.BARS), not tuned against the kernels.  Largest observed error over its
bar (MI355X), over the table:
    porl_adam_ema   params 0.051 (n1020-t10-lr0.01-b0.5-ema0.005-big)   m 0.082   v 0.016   target 0.084
                    (m, v, target: the 1M-float mixed row; every row is below a tenth of its bars)
    porl_ema        target 0.084 (n = 1048588), growing with n from 0.030 at n = 4: the largest of n draws
    porl_reduce_mean, random form: |error| 1.0e-8 at n = 1000 against a bound of 4.8e-5, 1.2e-9 against 3.1e-3 at 65537

What these tests found.  kernels.hpp and the header promised that porl_ema and the sweep fused into porl_adam_ema round
alike.  They did not: ema1 was written `t * omeb + ema_beta * p` and the compiler contracted it per kernel — the sweep
fused ema_beta * p onto the rounded t * omeb, ema_kernel fused t * omeb onto the rounded ema_beta * p.  With that form
the bit comparison below fails at every n >= 8 (14 of its 16 cases; two floats at n = 4 agree by chance).  ema1 now
states the sweep's form with __fmaf_rn.

Hand mutations (see tests/test_adam_fold_gpu.py for the table): sqrt left off bc2_sqrt fails test_adam_ema_per_element
on 16 rows, every one with lr > 0, a gradient that is not eps-dominated and 1 - b2^t away from 1 (it is 1 at t = 100000,
and at t = 1000 with b2 = 0.9); beta2 and 1 - beta2 swapped fails 30 of the 36 rows (the six it passes are the ~1e-12
gradients on v = 0: v' stays below its 1e-12 absolute bar either way and eps decides the step).
"""
import functools

import numpy as np
import pytest
import torch

from helpers import adam_cases as A
from porl_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = -7.25
TAIL = 8                       # sentinel floats behind the slice; `off` of them in front


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _framed(x, off):
    """x inside a longer device buffer: sentinels in [0, off) and in the TAIL floats behind it -> (buffer, slice)."""
    buf = torch.full((off + x.size + TAIL,), SENTINEL, dtype=torch.float32, device=DEV)
    buf[off:off + x.size] = _dev(x)
    return buf, buf[off:off + x.size]


def _sentinels_intact(buf, off, n):
    want = np.float32(SENTINEL).view(np.int32)
    b = _bits(buf)
    return (b[:off] == want).all() and (b[off + n:] == want).all()


def _adam_ema(p, g, m, v, t, d):
    from porl_amd.engine import adam_ema
    adam_ema(p, g, m, v, t, d["lr"], d["step"], d["betas"][0], d["betas"][1], A.EPS, 0.0 if t is None else d["ema_beta"])


@pytest.mark.parametrize("name", [r["name"] for r in A.TABLE])
def test_adam_ema_per_element(name):
    row = A.TABLE_BY_NAME[name]
    d, off, n = A.draw_row(row), row["off"], row["n"]
    ref = A.oracle(d)
    keys = ("p", "g", "m", "v") + (("t",) if d["t"] is not None else ())
    bufs, sl = {}, {}
    for k in keys:
        bufs[k], sl[k] = _framed(d[k], off)
        assert sl[k].data_ptr() % 16 == 0
    _adam_ema(sl["p"], sl["g"], sl["m"], sl["v"], sl.get("t"), d)
    torch.cuda.synchronize()
    got = {k: sl[k].cpu().numpy() for k in keys}
    e = A.excesses(dict(got, t=got.get("t")), ref)
    print(name, e)
    for k in keys:
        assert _sentinels_intact(bufs[k], off, n), f"{k}: a sentinel outside [off, off + n) was written"
        assert np.isfinite(got[k]).all(), k
    assert (got["g"].view(np.int32) == d["g"].view(np.int32)).all(), "g was written although no jobs are pending"
    assert max(e.values()) <= 1.0, e
    if d["lr"] == 0.0:
        assert (got["p"].view(np.int32) == d["p"].view(np.int32)).all()           # a zero step leaves p as it is, bit for bit
    if d["ema_beta"] == 0.0:
        assert (got["t"].view(np.int32) == d["t"].view(np.int32)).all()
    if d["ema_beta"] == 1.0:
        assert (got["t"] == got["p"]).all()


@pytest.mark.parametrize("ema_beta", (0.005, 0.05))
@pytest.mark.parametrize("n", A.SIZES)
def test_ema_matches_oracle_and_the_fused_sweep(n, ema_beta):
    """porl_ema against ema64 at the target's bar, and bit for bit against the target porl_adam_ema leaves for the same new
    parameters (lr = 0 keeps p, so both see the same source): kernels.hpp promises that both round alike."""
    d = A.draw(f"ema-{n}-{ema_beta}", n, 0.0, 10, ema_beta=ema_beta)
    off = 12
    tb, t = _framed(d["t"], off)
    pb, p = _framed(d["p"], off)
    from porl_amd.engine import ema
    ema(t, p, ema_beta)
    fused = {k: _framed(d[k], off) for k in ("p", "g", "m", "v", "t")}
    _adam_ema(*(fused[k][1] for k in ("p", "g", "m", "v", "t")), d)
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    e = A.excess(got, A.ema64(d["t"], d["p"], ema_beta), "t")
    print(n, ema_beta, e)
    assert _sentinels_intact(tb, off, n) and _sentinels_intact(pb, off, n)
    assert (_bits(p) == d["p"].view(np.int32)).all(), "the source was written"
    assert e <= 1.0
    assert (_bits(fused["p"][1]) == d["p"].view(np.int32)).all()
    assert (got.view(np.int32) == _bits(fused["t"][1])).all(), "porl_ema and the fused sweep round differently"


REDUCE_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 65537)      # width 32 up to 64 slabs, width 4 beyond


def _reduce_mean(x):
    out = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    N.check(N.lib().porl_reduce_mean(N.ptr(x), x.numel(), N.ptr(out), N.current_stream_ptr(x)), "porl_reduce_mean")
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert (res[1:] == np.float32(SENTINEL)).all()
    return res[0]


@functools.lru_cache(maxsize=None)
def _reduce_inputs(n):
    rng = np.random.default_rng(7000 + n)
    ints = rng.integers(1, 9, n) * np.where(rng.uniform(size=n) < 0.4, -1, 1)
    return ints.astype(np.float32), rng.standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("n", REDUCE_SIZES)
def test_reduce_mean(n):
    """Two forms.  EXACT: non-zero integer-valued inputs, |x| <= 8 — every partial sum is an integer below 2^24, so any
    summation order gives the same sum and the result must equal float32(sum) * float32(1 / n) bit for bit; an element
    left out, counted twice or read past the end changes it.  This form is the sharp one.  RANDOM: normal inputs against
    the fp64 mean within the order-independent bound (n - 1) 2^-24 sum|x| / n — loose by construction (it allows every
    summation order, and then some): it only says that the kernel averages real-valued data too."""
    ints, normal = _reduce_inputs(n)
    assert (ints != 0).all() and np.abs(ints).max() <= 8
    got = _reduce_mean(_dev(ints))
    want = np.float32(ints.astype(np.float64).sum()) * (np.float32(1.0) / np.float32(n))
    assert got.view(np.int32) == want.view(np.int32), (n, float(got), float(want))
    got = _reduce_mean(_dev(normal))
    x = normal.astype(np.float64)
    bound = (n - 1) * 2.0 ** -24 * np.abs(x).sum() / n
    print(n, abs(float(got) - x.mean()), bound)
    assert abs(float(got) - x.mean()) <= bound
