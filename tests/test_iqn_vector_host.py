"""IQN in the vectorised loop, without a GPU: the four new entry points turn down every bad argument before a launch
(through ctypes: the library loads without a GPU and judges its arguments before any device call, so host sentinel buffers
stay untouched), they are declared and exported, the numpy restatement of the fraction stream
(tests/helpers/iqn_vector_cases.py) has the properties the header claims, and the loop refuses what it can without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from helpers import iqn_vector_cases as VC
from porl_amd import _native as N

ENTRY_POINTS = ("porl_iqn_draw_taus", "porl_iqn_select_rows", "porl_iqn_act_rows", "porl_iqn_learn_sampled")

_Z = (C.c_float * 4096)(*([7.0] * 4096))
_Q = (C.c_float * 4096)(*([7.0] * 4096))
_OUT = (C.c_int64 * 64)(*([-7] * 64))


def _untouched():
    return all(v == 7.0 for v in _Q[:256]) and all(v == -7 for v in _OUT) and all(v == 7.0 for v in _Z[:256])


def _err():
    return N.lib().porl_last_error().decode()


# ---- porl_iqn_draw_taus ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over,word", [
    (dict(out=None), "null out"), (dict(use=-1), "use -1"), (dict(use=3), "use 3"), (dict(draw=1 << 32), "draw 4294967296"),
    (dict(first=-1), "first -1"), (dict(first=1 << 32), "first"), (dict(count=0), "count 0"), (dict(count=-5), "count -5"),
    (dict(first=(1 << 32) - 3, count=4), "count 4"),
])
def test_draw_taus_rejects_bad_arguments_before_a_launch(over, word):
    a = dict(seed=1, use=0, draw=0, first=0, count=8, out=_Q)
    a.update(over)
    rc = N.lib().porl_iqn_draw_taus(a["seed"], a["use"], a["draw"], a["first"], a["count"], a["out"], None)
    assert rc == -1 and word in _err(), (rc, _err())
    assert _untouched()


# ---- porl_iqn_select_rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over,word", [
    (dict(z=None), "null z"), (dict(q=None), "null q"), (dict(out=None), "null out"), (dict(n=0), "n 0"),
    (dict(n=(1 << 24) + 1), "n 16777217"), (dict(n_tau=0), "n_tau 0"), (dict(n_tau=257), "n_tau 257"),
    (dict(A=0), "n_actions 0"), (dict(A=65, ld=68, q_rs=65), "n_actions 65"), (dict(q_rs=4), "q_rs 4"), (dict(ld=4), "ld 4"),
    (dict(ld=132), "ld 132"), (dict(eps=-0.01), "epsilon"), (dict(eps=1.01), "epsilon"), (dict(eps=float("nan")), "epsilon"),
    (dict(env_offset=-1), "env_offset"), (dict(env_offset=(1 << 40) + 1), "env_offset"), (dict(t=1 << 32), "act-step"),
])
def test_select_rows_rejects_bad_arguments_before_a_launch(over, word):
    a = dict(z=_Z, ld=8, n=8, n_tau=4, A=5, eps=0.1, t=0, env_offset=0, q=_Q, q_rs=5, out=_OUT)
    a.update(over)
    rc = N.lib().porl_iqn_select_rows(a["z"], a["ld"], a["n"], a["n_tau"], a["A"], a["eps"], 1, a["t"], a["env_offset"], a["q"],
                                      a["q_rs"], a["out"], None)
    assert rc == -1 and word in _err(), (rc, _err())
    assert _untouched()


# ---- the engine's entry points -------------------------------------------------------------------------------------------
S_, A_, E_, H_, MAXB, MAXT = 7, 5, 10, 32, 4, 16


def _engine(bound):
    """An engine handle; bound: to host buffers — a refused call reads and writes none of them."""
    numel = [H_ * S_, H_, H_ * H_, H_, H_ * E_, H_, H_ * H_, H_, A_ * H_, A_]
    offs, off = [], 0
    for k in numel:
        offs.append(off)
        off += (k + 3) // 4 * 4
    cfg = N.IqnCfg(S_, A_, E_, H_, MAXB, MAXT, (C.c_int64 * 10)(*offs), off)
    lib, h = N.lib(), C.c_void_p()
    assert lib.porl_iqn_create(C.byref(cfg), C.byref(h)) == 0
    held = None
    if bound:
        ws = int(lib.porl_iqn_workspace_floats(h))
        held = [torch.full((k,), 3.0) for k in (off, off, off, off, off, ws, 8)]
        assert all(t.data_ptr() % 16 == 0 for t in held)
        b = N.QnetBuffers(*[C.c_void_p(t.data_ptr()) for t in held])
        assert lib.porl_iqn_bind(h, C.byref(b)) == 0, _err()
    return h, held


def _hp(step=1, max_norm=10.0):
    return N.IqnHyper(0.99, 1.0, max_norm, step, 5e-4, 0.9, 0.999, 1e-8)


def _act_rows(h, **over):
    a = dict(which=0, states=_Z, s_rs=S_, n=9, taus=None, n_tau=8, eps=0.1, t=0, env_offset=0, q=_Q, q_rs=A_, out=_OUT)
    a.update(over)
    return N.lib().porl_iqn_act_rows(h, a["which"], a["states"], a["s_rs"], a["n"], a["taus"], a["n_tau"], a["eps"], 1, a["t"],
                                     a["env_offset"], a["q"], a["q_rs"], a["out"], None)


def _learn_sampled(h, **over):
    a = dict(states=_Z, s_rs=S_, actions=_OUT, rewards=_Q, next_states=_Z, n_rs=S_, dones=_Q, n_rows=100, batch=4, draw=0,
             n_cur=8, n_tgt=8, hp=_hp())
    a.update(over)
    hp = None if a["hp"] is None else C.byref(a["hp"])
    return N.lib().porl_iqn_learn_sampled(h, a["states"], a["s_rs"], a["actions"], a["rewards"], a["next_states"], a["n_rs"],
                                          a["dones"], a["n_rows"], a["batch"], 1, a["draw"], a["n_cur"], a["n_tgt"], hp, None)


def test_null_and_unbound_engines_launch_nothing():
    assert _act_rows(None) == -1 and "null engine" in _err()
    assert _learn_sampled(None) == -1 and "null engine" in _err()
    h, _ = _engine(bound=False)
    try:
        assert _act_rows(h) == -3 and "porl_iqn_bind" in _err()
        assert _learn_sampled(h) == -3 and "porl_iqn_bind" in _err()
    finally:
        N.lib().porl_iqn_destroy(h)
    assert _untouched()


@pytest.mark.parametrize("over,word", [
    (dict(which=2), "which 2"), (dict(states=None), "null states"), (dict(q=None), "null q"), (dict(out=None), "null out"),
    (dict(n=0), "n 0"), (dict(n_tau=0), "n_tau 0"), (dict(n_tau=MAXT + 1), "n_tau 17"), (dict(s_rs=S_ - 1), "s_rs 6"),
    (dict(q_rs=A_ - 1), "q_rs 4"), (dict(eps=-0.5), "epsilon"), (dict(eps=1.5), "epsilon"), (dict(eps=float("nan")), "epsilon"),
    (dict(env_offset=-1), "env_offset"), (dict(t=1 << 32), "act-step"),
    (dict(env_offset=(1 << 29) - 8), "fraction stream"),          # (2^29 - 8 + 9) x 8 fractions pass 2^32
])
def test_act_rows_rejects_bad_arguments_before_a_launch(over, word):
    h, held = _engine(bound=True)
    try:
        assert _act_rows(h, **over) == -1 and word in _err(), _err()
    finally:
        N.lib().porl_iqn_destroy(h)
    assert _untouched() and all(bool((t == 3.0).all()) for t in held)


@pytest.mark.parametrize("over,word", [
    (dict(hp=None), "null hp"), (dict(states=None), "null states"), (dict(actions=None), "null actions"),
    (dict(rewards=None), "null rewards"), (dict(next_states=None), "null next_states"), (dict(dones=None), "null dones"),
    (dict(batch=0), "batch 0"), (dict(batch=MAXB + 1), "batch 5"), (dict(n_rows=3), "n_rows 3"),
    (dict(n_rows=(1 << 40) + 1), "n_rows"), (dict(s_rs=S_ - 1), "s_rs 6"), (dict(n_rs=S_ - 1), "n_rs 6"),
    (dict(n_cur=0), "n_cur 0"), (dict(n_cur=MAXT + 1), "n_cur 17"), (dict(n_tgt=0), "n_tgt 0"), (dict(n_tgt=MAXT + 1), "n_tgt 17"),
    (dict(draw=1 << 32), "draw 4294967296"), (dict(hp=_hp(step=0)), "adam step"), (dict(hp=_hp(max_norm=0.0)), "max_norm"),
])
def test_learn_sampled_rejects_bad_arguments_before_a_launch(over, word):
    h, held = _engine(bound=True)
    try:
        assert _learn_sampled(h, **over) == -1 and word in _err(), _err()
    finally:
        N.lib().porl_iqn_destroy(h)
    assert _untouched() and all(bool((t == 3.0).all()) for t in held)


def test_workspace_grew_by_the_fraction_regions_only():
    """Two regions of ru4(max_batch * max_tau) floats behind the regions the engine had."""
    B, T = MAXB, MAXT
    ru4 = lambda k: (k + 3) // 4 * 4
    Sp, Hp, Ap, R = ru4(S_), ru4(H_), ru4(A_), B * T
    before = 2 * ru4(B * Sp) + 2 * ru4(B) + ru4(2 * B) + 6 * ru4(B * Hp) + ru4(R * Hp) + 3 * (2 * ru4(R * Hp) + ru4(R * Ap)) + \
        ru4(R * Ap) + ru4(B) + 3 * ru4(R * Hp) + 2 * ru4(B * Hp) + 512
    h, _ = _engine(bound=False)
    try:
        assert N.lib().porl_iqn_workspace_floats(h) == before + 2 * ru4(R)
    finally:
        N.lib().porl_iqn_destroy(h)


def test_abi_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(", txt), name
        assert name in N.SYMBOLS and hasattr(N.lib(), name)
        decl = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", txt, re.S).group(1)
        assert len(decl.split(",")) == len(getattr(N.lib(), name).argtypes), name
    assert re.search(r"#define\s+PORL_ABI_VERSION\s+12\b", txt)                    # additions only
    assert N.ABI_VERSION == 12 and N.lib().porl_abi_version() == 12


# ---- the stream, restated ----------------------------------------------------------------------------------------------
def test_restated_mixer_agrees_with_itself():
    z = np.array([0, 1, 0x49514E5441554652, VC.M64], dtype=np.uint64)
    assert [int(v) for v in VC.sm64(z)] == [VC.sm64_int(int(v)) for v in z]
    assert VC.sm64_int(0x49514E5441554652) == VC.TAU_TAG


def test_stream_values_are_multiples_of_2_to_minus_24_in_the_unit_interval():
    for use in (0, 1, 2):
        t = VC.taus(11, use, 5, 0, 1 << 16)
        assert t.dtype == np.float32 and (t >= 0).all() and (t < 1).all()
        k = t.astype(np.float64) * 2.0 ** 24
        assert (k == np.floor(k)).all() and k.max() <= 2 ** 24 - 1
        assert (k == (VC.words(11, use, 5, 0, 1 << 16) >> np.uint64(40)).astype(np.float64)).all()       # the conversion is exact


def test_stream_uses_and_draws_do_not_collide():
    n = 1 << 12
    w = [VC.words(3, use, 9, 0, n) for use in (0, 1, 2)]
    for a in range(3):
        for b in range(a + 1, 3):
            assert not (w[a] == w[b]).any()                                           # equal (draw, e), two uses
    for use in (0, 1, 2):
        here, nxt = VC.words(3, use, 9, 0, n), VC.words(3, use, 10, 0, n)
        assert len(np.unique(np.concatenate([here, nxt]))) == 2 * n                   # (draw, e) against (draw + 1, 0..)
        last = VC.words(3, use, 9, (1 << 32) - 1, 1)                                  # the largest e of a draw
        assert last[0] != nxt[0] and last[0] not in here
    assert not (VC.words(3, 0, 9, 0, n) == VC.words(4, 0, 9, 0, n)).any()            # another seed


def test_stream_moments():
    """2^16 draws: the mean within 4 standard errors of 1/2 (sigma / sqrt(n), sigma^2 = 1/12), the variance within 4 of
    1/12 (the standard error of a sample variance of U(0,1): sqrt((1/80 - 1/144) / n) = sqrt(1 / (180 n)))."""
    n = 1 << 16
    for use in (0, 1, 2):
        t = VC.taus(2024, use, 1, 0, n).astype(np.float64)
        assert abs(t.mean() - 0.5) <= 4 * np.sqrt(1 / 12 / n), (use, t.mean())
        assert abs(t.var() - 1 / 12) <= 4 * np.sqrt(1 / 180 / n), (use, t.var())


def test_restated_head_is_a_sequential_fp32_sum():
    z = np.array([[1.0], [2.0 ** -24], [2.0 ** -24], [-1.0]], dtype=np.float32)
    assert VC.mean_rows_f32(z, 4)[0, 0] == 0.0                    # ((1 + e) + e) - 1 in fp32: both e are lost
    assert VC.mean_rows_f32(z[::-1].copy(), 4)[0, 0] == np.float32(2.0 ** -25)       # ((-1 + e) + e) + 1 = 2e; / 4


# ---- the Python surface --------------------------------------------------------------------------------------------------
def test_python_surface_refuses_without_a_device(tmp_path):
    from porl_amd import engine as E
    from porl_amd.train.dqn_trainer import DQNTrainer
    from porl_amd.train.iqn_trainer import IQNTrainer
    from porl_amd.train.vector_online import train_vectorized_iqn
    assert callable(E.iqn_draw_taus) and callable(E.iqn_select_rows) and callable(E.IqnEngine.act_rows)
    assert callable(E.IqnEngine.learn_sampled) and callable(IQNTrainer.train_vectorized_iqn)
    with pytest.raises(RuntimeError, match="HIP device"):
        E.iqn_select_rows(torch.zeros(8, 5), 4, 0.0, 0, 0)
    t = DQNTrainer(8, 5, 0.99, log_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="the loop of IQNTrainer"):
        train_vectorized_iqn(t, None, 4)
    assert not hasattr(t, "_vec_steps")
    with pytest.raises(N.NativeError, match="no CPU path"):
        IQNTrainer(8, 5, 0.99, log_dir=str(tmp_path))
