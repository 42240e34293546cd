"""Cases of the fp32 encoder tests, shared by tests/test_fp32_oracle.py (the rule, on the CPU) and
tests/test_encoder_fp32_gpu.py (the kernels): shapes, weights, inputs and the fp64 / fp32 oracle pair of each case,
computed once per process and never modified afterwards."""
import functools
import os
import sys
import time
from collections import namedtuple

import numpy as np
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "oracle"))
import bf16_accept as BA          # noqa: E402
import fasternet_oracle as FO     # noqa: E402

WSEED, ISEED = 11, 21
CAP = BA.CAP_REL_FP32
STAGE_TAPS = ("stages.0", "stages.2")
FP32_TAPS = ("pooled", "avgpool_pre_head", "features")

Case = namedtuple("Case", "name ab db B embed depths n_div mlp_ratio")
REF_ARCH = dict(embed=96, depths=(1, 2), n_div=4, mlp_ratio=2.0)
CASES = (
    Case("40x64-b3", 40, 64, 3, **REF_ARCH),
    Case("84x84-b5", 84, 84, 5, **REF_ARCH),
    Case("360x256-b2", 360, 256, 2, **REF_ARCH),
    Case("360x256-b7", 360, 256, 7, **REF_ARCH),
    Case("40x64-e64-d21-b2", 40, 64, 2, 64, (2, 1), 4, 2.0),
    # mlp_ratio 3.0: hidden widths 96 and 192, both multiples of the GEMM's 32-wide K tile, so BatchNorm + ReLU still fold
    # into W2's operand staging (cp = 16 and 32, n_div 2, two blocks)
    Case("40x64-e32-d11-r3-b2", 40, 64, 2, 32, (1, 1), 2, 3.0),
    # mlp_ratio 2.25: hidden widths 72 and 144, no multiples of 32: the fold condition is false, BatchNorm runs as a sweep
    Case("40x64-e32-d11-r2.25-b2", 40, 64, 2, 32, (1, 1), 2, 2.25),
)
BY_NAME = {c.name: c for c in CASES}
SMALL = tuple(c.name for c in CASES if c.ab < 360)


def make_module(case, device=None):
    from porl_amd.agent.fasternet import FasterNet
    torch.manual_seed(WSEED)
    m = FasterNet(3, 256, embed_dim=case.embed, depths=case.depths, n_div=case.n_div, mlp_ratio=case.mlp_ratio,
                  compute_dtype="fp32", angle_bins=case.ab, dist_bins=case.db, max_batch=case.B)
    return m if device is None else m.to(device)


@functools.lru_cache(maxsize=None)
def weights(name):
    return {k: v.cpu().numpy().copy() for k, v in make_module(BY_NAME[name]).state_dict().items()}


def inputs(name):
    """Lidar states and DropPath factors (fresh copies: the forward clamps the states in place)."""
    c = BY_NAME[name]
    return BA.make_inputs(c.ab, c.B, ISEED, blocks=sum(c.depths))


def oracle(name, training=True, **kw):
    """One forward_faithful(mode=None) run: (taps incl. "features", running statistics afterwards).  Eval runs start from
    the initial running statistics unless `stats` is given."""
    c = BY_NAME[name]
    sd = weights(name)
    st, scale = inputs(name)
    stats = kw.pop("stats", None)
    stats = {k: v.copy() for k, v in (stats if stats is not None else sd).items() if "running" in k}
    taps = {}
    taps["features"] = FO.forward_faithful(sd, stats, st, training, scale if training else None, mode=None, taps=taps,
                                           angle_bins=c.ab, dist_bins=c.db, depths=c.depths, n_div=c.n_div, **kw)
    for k in ("patch_embed", "stages.1"):           # not compared: the cached runs keep only what the tests read
        taps.pop(k, None)
    return taps, stats


@functools.lru_cache(maxsize=None)
def oracle_train(name, accum):
    return oracle(name, True, accum={"fp64": np.float64, "fp32": np.float32}[accum])


@functools.lru_cache(maxsize=None)
def oracle_pair(name):
    """{"fp64" | "fp32": {"train": taps, "eval": taps (behind the train forward), "stats": after the train forward}}, and
    the seconds it took."""
    t0 = time.time()
    out = {}
    for key, accum in (("fp64", np.float64), ("fp32", np.float32)):
        train, stats = oracle_train(name, key)
        ev, _ = oracle(name, False, accum=accum, stats=stats)
        out[key] = {"train": train, "eval": ev, "stats": stats}
    return out, time.time() - t0


def compare(got, orc, cap=CAP):
    """`got` against the oracle pair under the fp32 rule -> list of rejected quantities; prints every figure first."""
    bad = []
    ref, ref32 = orc["fp64"], orc["fp32"]

    def check(label, g, r, r32, **kw):
        ok, rep = BA.accept(g, r, r32, kind="rel", cap=cap, **kw)
        print(BA.fmt(label, rep))
        if not ok:
            bad.append((label, rep["why"]))

    for phase in ("train", "eval"):
        for k in STAGE_TAPS + FP32_TAPS:
            check(f"{phase} {k}", got[phase][k], ref[phase][k], ref32[phase][k])
    s, s32 = ref["stats"], ref32["stats"]
    for k in sorted(s):
        if k.endswith("running_var"):
            check(k, got["stats"][k], s[k], s32[k])
            km = k.replace("running_var", "running_mean")
            # channel means sit near zero: on the scale of the layer's largest standard deviation
            check(km, got["stats"][km], s[km], s32[km], scale=float(np.sqrt(s[k].max())))
        elif k.endswith("num_batches_tracked"):
            if int(got["stats"][k]) != int(s[k]) or int(s[k]) != 1:
                bad.append((k, [f"{int(got['stats'][k])} != {int(s[k])}"]))
    return bad
