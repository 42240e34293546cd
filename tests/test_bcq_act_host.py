"""The BCQ-constrained batched act without a GPU: porl_bcq_select and porl_qnet_act_rows_bcq turn down every bad argument
before a launch (through ctypes: the library loads without a GPU and judges its arguments before any device call, so host
sentinel buffers stay untouched), the two symbols are declared and exported, the Python surface refuses CPU tensors, and
the numpy restatement (tests/helpers/bcq_act_cases.py) alone has the properties of the rule and meets the condition the GPU
tests rely on: few rows with a probability within MARGIN of the threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from helpers import bcq_act_cases as BC
from porl_amd import _native as N

ENTRY_POINTS = ("porl_bcq_select", "porl_qnet_act_rows_bcq")

_Q = (C.c_float * 4096)(*([7.0] * 4096))
_Z = (C.c_float * 4096)(*([7.0] * 4096))
_M = (C.c_float * 4096)(*([7.0] * 4096))
_OUT = (C.c_int64 * 64)(*([-7] * 64))


def _select(**over):
    a = dict(q=_Q, q_rs=5, z=_Z, z_rs=5, A=5, n=8, thr=0.1, eps=0.1, env_offset=0, t=0, mask=_M, out=_OUT)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_bcq_select(a["q"], a["q_rs"], a["z"], a["z_rs"], a["A"], a["n"], a["thr"], a["eps"], 1, a["env_offset"],
                             a["t"], a["mask"], a["out"], None)
    return rc, lib.porl_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(q=None), "null action values"), (dict(z=None), "null behaviour logits"), (dict(out=None), "null out"),
    (dict(n=0), "n 0"), (dict(n=(1 << 24) + 1), "n 16777217"), (dict(A=0), "n_actions 0"),
    (dict(A=65, q_rs=65, z_rs=65), "n_actions 65"), (dict(q_rs=4), "q_rs"), (dict(z_rs=4), "z_rs"),
    (dict(z_rs=(1 << 24) + 1), "z_rs"),
    (dict(thr=-0.01), "threshold"), (dict(thr=1.01), "threshold"), (dict(thr=float("nan")), "threshold"),
    (dict(thr=float("inf")), "threshold"),
    (dict(eps=-0.01), "epsilon"), (dict(eps=1.01), "epsilon"), (dict(eps=float("nan")), "epsilon"),
    (dict(env_offset=-1), "env_offset"), (dict(env_offset=(1 << 40) + 1), "env_offset"), (dict(t=(1 << 54) + 1), "act-step"),
    (dict(mask=_Q), "mask must not be"), (dict(mask=_Z), "mask must not be"),
])
def test_bcq_select_rejects_bad_arguments_before_a_launch(over, word):
    rc, msg = _select(**over)
    assert rc == -1 and word in msg, (rc, msg)
    assert all(v == 7.0 for v in _M[:64]) and all(v == -7 for v in _OUT)          # nothing was written


def test_act_rows_bcq_rejects_before_any_launch():
    lib = N.lib()

    def call(h, beh):
        return lib.porl_qnet_act_rows_bcq(h, beh, 0, _Z, 8, 4, _Q, 5, _Z, 5, 0.1, 0.1, 1, 0, 0, None, _OUT, None)

    assert call(None, None) == -1 and "null engine" in lib.porl_last_error().decode()
    cfg = N.QnetCfg(8, 5, 2, (C.c_int32 * 8)(64, 64), 32)
    h = C.c_void_p()
    assert lib.porl_qnet_create(C.byref(cfg), C.byref(h)) == 0
    try:                                                                           # unbound engines launch nothing
        assert call(h, None) != 0 and "porl_qnet_bind" in lib.porl_last_error().decode()
        assert call(h, h) != 0 and "porl_qnet_bind" in lib.porl_last_error().decode()
    finally:
        lib.porl_qnet_destroy(h)
    assert all(v == -7 for v in _OUT)


def test_abi_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(", txt), name
        assert name in N.SYMBOLS and hasattr(N.lib(), name)
        decl = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", txt, re.S).group(1)
        assert len(decl.split(",")) == len(getattr(N.lib(), name).argtypes), name
    assert N.lib().porl_abi_version() == N.ABI_VERSION                             # additions only


def test_python_surface_refuses_without_a_device(tmp_path):
    from porl_amd import engine as E
    from porl_amd import evaluate
    from porl_amd.train import vector_offline as VO
    from porl_amd.train.bcq_trainer import BCQTrainer
    from porl_amd.train.c51_trainer import C51Trainer
    from porl_amd.train.cql_trainer import CQLTrainer
    assert callable(E.bcq_select) and callable(E.QnetEngine.act_rows_bcq) and callable(evaluate.evaluate_discrete)
    assert callable(BCQTrainer.act_rows) and callable(BCQTrainer.train_offline_device) and callable(CQLTrainer.train_offline_device)
    with pytest.raises(RuntimeError, match="HIP device"):
        E.bcq_select(torch.zeros(4, 5), torch.zeros(4, 5), 0.1, 0.0, 0, 0)
    kw = dict(log_dir=str(tmp_path))
    t = C51Trainer(8, 5, 0.99, **kw)                          # (PER and IQN trainers need a device to exist: the GPU tests)
    with pytest.raises(NotImplementedError, match="train_vectorized_dist"):
        VO.train_offline_device(t, None, 4)
    assert not hasattr(t, "_draws")


# ---- the restatement alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,n,sigma,threshold", BC.grid())
def test_restated_rule_over_the_grid(A, n, sigma, threshold):
    q, z = BC.tables(A, n, sigma, threshold)
    assert q.shape == z.shape == (n, A) and q.dtype == z.dtype == np.float32
    # the condition the GPU tests rely on: few rows sit within the margin of the threshold
    close = BC.near(z, threshold)
    print(f"A {A} n {n} sigma {sigma} threshold {threshold}: {int(close.sum())} of {n} rows within {BC.MARGIN} of the threshold")
    assert close.mean() <= 0.02
    m32, m64 = BC.mask_f32(z, threshold), BC.mask_f64(z, threshold)
    assert np.array_equal(m32[~close], m64[~close])             # 4e-6 of fp32 rounding stays inside the margin
    pick, v = BC.select(q, m32)
    rows = np.arange(n)
    some = m32.any(axis=1) & ~np.isnan(q).any(axis=1)           # (a NaN value is the maximum, allowed or not: ROW_NAN)
    assert bool((m32[rows, pick][some] == 1.0).all())           # the chosen action is allowed whenever any action is
    plain, _ = BC.select(q, np.ones_like(m32))
    if threshold == 0.0:
        assert bool(m32.all()) and np.array_equal(pick, plain)  # threshold 0: the plain arg-max
    if n >= 255:
        assert not close[[BC.ROW_TIE, BC.ROW_NAN, BC.ROW_NONE, BC.ROW_ONE]].any()
        if A >= 2 and m32[BC.ROW_TIE].all():                    # an exact tie: the lower index
            top = np.flatnonzero(q[BC.ROW_TIE] == q[BC.ROW_TIE].max())
            assert len(top) == 2 and pick[BC.ROW_TIE] == top[0]
        assert pick[BC.ROW_NAN] == BC.nan_column(A)             # a NaN in v is the maximum
        if BC.has_none(A, threshold):                           # every action masked, |q| < 512: action 0
            assert not m32[BC.ROW_NONE].any() and bool((np.abs(q[BC.ROW_NONE]) < 512).all())
            assert bool((v[BC.ROW_NONE] == np.float32(-1e10)).all()) and pick[BC.ROW_NONE] == 0
        if BC.has_one(A, threshold):                            # exactly one allowed, and not the plain arg-max
            assert m32[BC.ROW_ONE].sum() == 1.0
            assert m32[BC.ROW_ONE, pick[BC.ROW_ONE]] == 1.0 and pick[BC.ROW_ONE] != plain[BC.ROW_ONE]


def test_the_planted_rows_exist_somewhere():
    assert any(BC.has_none(A, th) for A in BC.ACTIONS for th in BC.THRESHOLDS)
    assert all(BC.has_one(A, th) for A in BC.ACTIONS[1:] for th in BC.THRESHOLDS[1:])
    assert not any(BC.has_none(A, 0.0) or BC.has_one(A, 0.0) for A in BC.ACTIONS)
