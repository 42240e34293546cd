"""Acting and learning of the distributional trainers in the vectorised loop, without a GPU: porl_dist_select turns down
every bad argument before a launch (through ctypes: the library loads without a GPU and judges its arguments before any
device call, so host sentinel buffers stay untouched), the new symbols are declared and exported, and the numpy reference
(tests/helpers/dist_vector_cases.py) alone meets the conditions the GPU tests rely on."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from helpers import dist_vector_cases as VC
from porl_amd import _native as N

ENTRY_POINTS = ("porl_dist_select", "porl_qnet_act_rows_dist", "porl_qnet_dist_learn_sampled")

_Z = (C.c_float * 4096)(*([7.0] * 4096))
_Q = (C.c_float * 4096)(*([7.0] * 4096))
_SUP = (C.c_float * 256)()
_OUT = (C.c_int64 * 64)(*([-7] * 64))


def _head(kind=0, n_actions=5, n_sub=51, support=None, v_min=0.0, v_max=0.0):
    if kind == 1 and support is None:
        support, v_min, v_max = C.addressof(_SUP), -10.0, 10.0
    return N.DistHead(kind, n_actions, n_sub, 1.0, v_min, v_max, support)


def _select(**over):
    a = dict(z=_Z, z_rs=255, head=_head(), n=8, q=_Q, q_rs=5, eps=0.1, env_offset=0, t=0, out=_OUT)
    a.update(over)
    lib = N.lib()
    head = a["head"] if a["head"] is None else C.byref(a["head"])
    rc = lib.porl_dist_select(a["z"], a["z_rs"], head, a["n"], a["q"], a["q_rs"], a["eps"], 1, a["env_offset"], a["t"],
                              a["out"], None)
    return rc, lib.porl_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(z=None), "null outputs"), (dict(head=None), "null head"), (dict(q=None), "null action values"),
    (dict(out=None), "null out"), (dict(n=0), "n 0"), (dict(n=(1 << 24) + 1), "n 16777217"), (dict(q_rs=4), "q_rs"),
    (dict(z_rs=254), "z_rs"), (dict(z_rs=(1 << 24) + 1), "z_rs"),
    (dict(eps=-0.01), "epsilon"), (dict(eps=1.01), "epsilon"), (dict(eps=float("nan")), "epsilon"),
    (dict(env_offset=-1), "env_offset"), (dict(env_offset=(1 << 40) + 1), "env_offset"), (dict(t=(1 << 54) + 1), "act-step"),
    (dict(head=_head(kind=2)), "unknown head kind 2"), (dict(head=_head(kind=-1)), "unknown head kind"),
    (dict(head=_head(n_sub=0)), "n_sub 0"), (dict(head=_head(n_sub=257), z_rs=5 * 257), "n_sub 257"),
    (dict(head=_head(n_actions=65, n_sub=4), z_rs=260, q_rs=65), "n_actions 65"),
    (dict(head=_head(n_actions=0)), "n_actions 0"),
    (dict(head=_head(kind=1, n_sub=1), z_rs=5), "C51 needs n_sub >= 2"),
    (dict(head=N.DistHead(1, 5, 51, 0.0, -10.0, 10.0, None)), "C51 needs the support"),
])
def test_dist_select_rejects_bad_arguments_before_a_launch(over, word):
    rc, msg = _select(**over)
    assert rc == -1 and word in msg, (rc, msg)
    assert all(v == 7.0 for v in _Q[:64]) and all(v == -7 for v in _OUT)         # nothing was written


def test_engine_entry_points_reject_before_any_launch():
    lib = N.lib()
    hp = N.QnetHyper(0.99, 0.0, 1.0 / 4, 1, 5e-4, 0.9, 0.999, 1e-8)
    head = _head()
    assert lib.porl_qnet_act_rows_dist(None, 0, _Z, 8, 4, C.byref(head), _Q, 5, 0.1, 1, 0, 0, _OUT, None) == -1
    assert "null engine" in lib.porl_last_error().decode()
    assert lib.porl_qnet_dist_learn_sampled(None, _Z, 8, _OUT, _Q, _Z, 8, _Q, 100, 1, 0, 4, C.byref(hp), C.byref(head), None) == -1
    assert "null engine" in lib.porl_last_error().decode()
    cfg = N.QnetCfg(8, 255, 2, (C.c_int32 * 8)(64, 64), 32)
    h = C.c_void_p()
    assert lib.porl_qnet_create(C.byref(cfg), C.byref(h)) == 0
    try:                                                                          # an unbound engine launches nothing
        assert lib.porl_qnet_act_rows_dist(h, 0, _Z, 8, 4, C.byref(head), _Q, 5, 0.1, 1, 0, 0, _OUT, None) != 0
        assert "porl_qnet_bind" in lib.porl_last_error().decode()
        assert lib.porl_qnet_dist_learn_sampled(h, _Z, 8, _OUT, _Q, _Z, 8, _Q, 100, 1, 0, 4, C.byref(hp), C.byref(head), None) != 0
        assert "porl_qnet_bind" in lib.porl_last_error().decode()
    finally:
        lib.porl_qnet_destroy(h)


def test_abi_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(", txt), name
        assert name in N.SYMBOLS and hasattr(N.lib(), name)
        decl = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", txt, re.S).group(1)
        assert len(decl.split(",")) == len(getattr(N.lib(), name).argtypes), name
    assert re.search(r"#define\s+PORL_ABI_VERSION\s+12\b", txt)                    # additions only
    assert N.ABI_VERSION == 12 and N.lib().porl_abi_version() == 12


def test_python_surface_refuses_without_a_device(tmp_path):
    from porl_amd import engine as E
    from porl_amd.train.c51_trainer import C51Trainer
    from porl_amd.train.dist_trainer import DistTrainerBase
    from porl_amd.train.dqn_trainer import DQNTrainer
    from porl_amd.train.vector_online import train_vectorized_dist
    assert callable(E.dist_select) and callable(E.QnetEngine.act_rows_dist) and callable(E.QnetEngine.dist_learn_sampled)
    assert callable(DistTrainerBase.train_vectorized_dist) and C51Trainer.train_vectorized_dist is DistTrainerBase.train_vectorized_dist
    with pytest.raises(RuntimeError, match="HIP device"):
        E.dist_select(torch.zeros(4, 255), _head(), 0.0, 0, 0)
    t = DQNTrainer(8, 5, 0.99, log_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="C51Trainer and QRDQNTrainer"):
        train_vectorized_dist(t, None, 4)
    assert not hasattr(t, "_vec_steps")


# ---- the reference alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,A,NS,sigma", VC.cases())
def test_reference_meets_what_the_gpu_tests_rely_on(kind, A, NS, sigma):
    z = VC.logits(kind, A, NS, sigma)
    assert z.shape == (VC.N_ROWS, A * NS) and VC.N_ROWS == 1029
    support = torch.linspace(-VC.V_MAX, VC.V_MAX, NS).numpy() if kind == VC.C51 else None
    want = VC.oracle(kind, z, A, NS, support)
    got = VC.values_f32(kind, z, A, NS, support)
    assert got.dtype == np.float32 and got.shape == want.shape == (VC.N_ROWS, A)
    gap = VC.top2_gap(want)
    close = gap < VC.GAP
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"kind {kind} A {A} NS {NS} sigma {sigma}: {int(close.sum())} of {len(gap)} rows below the gap, "
          f"restatement max |error| {err:.3e}")
    assert close.mean() <= 0.01                                                   # few rows are left out
    assert np.array_equal(got.argmax(axis=1)[~close], want.argmax(axis=1)[~close])
    assert 8 * err < 1e-4                                                         # the GPU test's bar stays below the gap
