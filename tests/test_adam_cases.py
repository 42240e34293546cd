"""CPU checks of tests/helpers/adam_cases.py, the yardstick of tests/test_adam_sweep_gpu.py and tests/test_adam_fold_gpu.py:
the fp32 control of every case inside the four bars against the fp64 oracle, every mutated control outside them by a
factor of 100 (the bars are sharp before a GPU is involved), adam64 / ema64 against torch in float64, the coverage of
the sweep table computed from the table, and the arithmetic of the fold cases' expected plans."""
import functools

import numpy as np
import pytest
import torch

from helpers import adam_cases as A
from helpers import qstep_cases as Q


@functools.lru_cache(maxsize=None)
def _host(name):
    d = A.draw_host(name)
    return d, A.oracle(d)


# ---- part 1: the fp32 control is inside the bars ------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r["name"] for r in A.TABLE])
def test_fp32_control_passes_the_bars_on_the_sweep_table(name):
    d = A.draw_row(A.TABLE_BY_NAME[name])
    e = A.excesses(A.control(d), A.oracle(d))
    print(name, e)
    assert set(e) == ({"p", "m", "v", "t"} if d["t"] is not None else {"p", "m", "v"})
    assert max(e.values()) <= 1.0, e


@pytest.mark.parametrize("name", list(A.HOST_CASES))
def test_fp32_control_passes_the_bars_on_the_host_cases(name):
    d, ref = _host(name)
    e = A.excesses(A.control(d), ref)
    print(name, e)
    assert max(e.values()) <= 1.0, e


def test_inputs_are_in_the_regime_the_bars_were_stated_for():
    for name in A.HOST_CASES:
        d, _ = _host(name)
        assert np.abs(d["m"]).max() <= 3e-3 and np.sqrt(d["v"]).min() >= 5e-3
        assert np.abs(d["p"]).max() <= A.P_MAX and (d["t"] is None or np.abs(d["t"]).max() <= A.P_MAX)
        assert 0 <= d["lo"] < d["hi"] <= d["n"]
    d = A.draw("kinds", 4000, 1e-2, 1, gkind="mixed")
    k = np.arange(4000) % 5
    assert (d["g"][k == 1] == 0).all() and np.abs(d["g"][k == 2]).min() >= 500 and np.abs(d["g"][k == 3]).max() <= 2e-12
    assert (d["v"][k == 3] == 0).all() and (d["m"][k == 3] == 0).all() and (d["v"][k != 3] > 0).all()
    g = d["g"][k == 4]
    assert (np.abs(g) == np.float32(1e-22)).all() and (g * g < np.finfo(np.float32).tiny).all()     # g^2 underflows: subnormal in fp32
    # the eps-dominated denominator: sqrt(v') is below eps there, so a kernel that dropped eps would step by ~lr
    ref = A.oracle(d)
    assert (np.sqrt(ref["v"][k == 3]) < 0.01 * A.EPS).all()
    assert np.abs(ref["p"] - d["p"])[k == 3].max() < 1e-3 * d["lr"]


# ---- part 2: the mutated controls are outside them ------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", list(A.MUTATIONS))
@pytest.mark.parametrize("name", list(A.HOST_CASES))
def test_mutated_control_fails_a_bar(name, mutation):
    d, ref = _host(name)
    fn, needs_target, must_fail = A.MUTATIONS[mutation]
    if needs_target and d["t"] is None:
        # not a skip: the mutation does not exist without a target, and says so by leaving the control as it is
        assert A.HOST_CASES[name][2] is False
        return
    e = A.excesses(fn(d), ref)
    print(name, mutation, e)
    for q in must_fail:
        assert e[q] >= A.SHARP, (q, e)
    if must_fail == ("t",):             # a Polyak defect is seen by the target's bar alone: nothing else tells it
        assert max(e[q] for q in ("p", "m", "v")) <= 1.0, e


def test_every_mutation_applies_somewhere():
    for mutation, (_, needs_target, _) in A.MUTATIONS.items():
        assert any(t or not needs_target for _, _, t, _, _ in A.HOST_CASES.values()), mutation
    assert sum(t for _, _, t, _, _ in A.HOST_CASES.values()) >= 3


# ---- part 3: the oracle against torch --------------------------------------------------------------------------------------
def test_adam64_matches_torch_adam():
    rng = np.random.default_rng(11)
    for betas in A.BETA_PAIRS:
        p0 = rng.uniform(-0.5, 0.5, (9, 4))
        p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        opt = torch.optim.Adam([p], lr=A.LR, betas=betas, eps=A.EPS)
        mine, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
        for step in range(1, 5):
            g = rng.standard_normal(p0.shape) * 10.0 ** rng.integers(-12, 4, p0.shape)
            p.grad = torch.from_numpy(g.copy())
            opt.step()
            mine, m, v = Q.adam64(mine, g, m, v, lr=A.LR, step=step, betas=betas, eps=A.EPS)
            st = opt.state[p]
            np.testing.assert_allclose(mine, p.detach().numpy(), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-18)
            np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-30)


def test_ema64_matches_torch_lerp_form():
    rng = np.random.default_rng(12)
    t, p = rng.uniform(-0.5, 0.5, 100), rng.uniform(-0.5, 0.5, 100)
    for beta in (0.0, 0.005, 0.05, 1.0):
        want = (1.0 - beta) * torch.from_numpy(t) + beta * torch.from_numpy(p)        # util/util.py:54-56 in float64
        # beta and 1 - beta are rounded to fp32 on the way in: relative 2^-24 each
        np.testing.assert_allclose(A.ema64(t, p, beta), want.numpy(), rtol=0, atol=2.0 ** -23)
    assert (A.ema64(t, p, 0.0) == t).all() and (A.ema64(t, p, 1.0) == p).all()


def test_scalars_are_rounded_as_adam_launch_rounds_them():
    s = A.scalars(3e-3, 7)
    assert s["step_size"] == np.float32(3e-3 / (1 - 0.9 ** 7)) and s["bc2_sqrt"] == np.float32(np.sqrt(1 - 0.999 ** 7))
    assert all(x.dtype == np.float32 for x in s.values())
    assert s["omb2"] == np.float32(1.0 - 0.999) and s["omb2"] != np.float32(1.0) - np.float32(0.999)


# ---- the table and the fold cases -------------------------------------------------------------------------------------------
def test_sweep_table_covers_every_axis_value():
    assert 24 <= len(A.TABLE) <= 48
    for key, values in (("n", A.SIZES), ("step", A.STEPS), ("lr", A.LRS), ("betas", A.BETA_PAIRS), ("ema_beta", A.EMA_BETAS),
                        ("gkind", A.G_KINDS), ("off", A.OFFSETS)):
        assert {r[key] for r in A.TABLE} == set(values), key
    assert sum(r["n"] == max(A.SIZES) for r in A.TABLE) == 1
    assert all(r["off"] % 4 == 0 and r["n"] % 4 == 0 for r in A.TABLE)
    # sizes on either side of a 256-float4 block, and more than one block
    assert {1020, 1024, 1028} <= set(A.SIZES) and max(A.SIZES) > 2 ** 20
    # a target meets lr = 0 (porl_ema's bit comparison rests on it) and every gradient kind meets a target
    assert any(r["lr"] == 0 and r["ema_beta"] is not None for r in A.TABLE)
    assert {r["gkind"] for r in A.TABLE if r["ema_beta"] is not None} == set(A.G_KINDS)


def test_fold_case_plans_add_up():
    """The expected plans of tests/test_adam_fold_gpu.py: every folded job owns a skip range, and the block count follows
    from the jobs' sizes — recomputed here for the cases where all jobs are known from (S, H, B, D) alone."""
    assert A.PLAN == ("regions", "fold32", "fold4", "unfolded", "skips", "reduce_blocks")
    for name, (S, H, L, B, ln, D, pv, pp, why) in A.FOLD_CASES.items():
        assert why and B <= 1100
        for plan in (pv, pp):
            r = dict(zip(A.PLAN, plan))
            assert r["skips"] == r["fold32"] + r["fold4"], name
            assert r["reduce_blocks"] >= r["fold32"] + r["fold4"] + r["unfolded"], name
        assert pp[3] == 2 and pv[3] == (0 if ln else 1), name                 # stats[1:3]; stats[0] (a kernel's under LayerNorm)
    cdiv = lambda a, b: -(-a // b)
    # width4: head weights 64 outputs / 4 per block for each twin, two biases, one statistic; 60 log_std outputs / 4 + 2
    S, H, L, B, ln, D, pv, pp, _ = A.FOLD_CASES["width4"]
    assert cdiv(B, 8) > 64 and cdiv(B, 4) > 64
    assert pv[5] == 2 * cdiv(H, 4) + 2 + 1 and pp[5] == cdiv(D, 4) + 2
    S, H, L, B, ln, D, pv, pp, _ = A.FOLD_CASES["slabs16"]
    assert cdiv(B, 8) == 16 and pv[0] == 6
    S, H, L, B, ln, D, pv, pp, _ = A.FOLD_CASES["slabs17"]
    assert cdiv(B, 8) == 17 and pv[0] == 4 and pv[5] == 2 * cdiv(H, 32) + 2 + 1 and B % 64
    S, H, L, B, ln, D, pv, pp, _ = A.FOLD_CASES["tiles18"]
    assert cdiv(B, 64) == 18 and pv[5] == 2 * cdiv(H, 4) + 2 + 1
    S, H, L, B, ln, D, pv, pp, _ = A.FOLD_CASES["h50"]
    assert H % 4 and pv[5] == 2 * cdiv(H, 32) + 2 + 1 + 2 * (cdiv(H * S, 32) + cdiv(H, 32))
    assert pp[5] == cdiv(D, 32) + 2 + cdiv(D * H, 32) + cdiv(D, 32) + cdiv(H * S, 32) + cdiv(H, 32)
