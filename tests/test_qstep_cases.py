"""CPU checks of tests/helpers/qstep_cases.py, the yardstick of tests/test_qstep_gpu.py: the hand-derived fp64 step
against torch autograd in float64, adam64 against torch.optim.Adam, the margins of every case (B distinct decided rows:
the GPU comparison leaves no row out), the coverage of the kernels' selectors computed from the case list, and the fp32
control's own error, which bounds how badly conditioned a case may be."""
import functools
import math

import numpy as np
import pytest
import torch

from helpers import qstep_cases as Q

NAMES = [c["name"] for c in Q.CASES]


@functools.lru_cache(maxsize=None)
def _made(name):
    d = Q.make(Q.BY_NAME[name])
    return d, Q.step64(d), Q.step32(d)


def _t64(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


def _net(params, x):
    h = x
    n = len(params) // 2
    for l in range(n):
        h = h @ params[2 * l].T + params[2 * l + 1]
        if l < n - 1:
            h = torch.relu(h)
    return h


def _autograd(d):
    """The step as the trainers write it (cql_trainer / dqn_per_trainer / bcq.py), float64, on the CPU."""
    case, v = d["case"], Q.variant(d["case"])
    B, A = case["B"], case["A"]
    idx = d["idx"]
    online = [_t64(p).requires_grad_(True) for p in d["online"]]
    target = [_t64(p) for p in d["target"]]
    s, sn = _t64(d["states"][idx]), _t64(d["next_states"][idx])
    a = torch.from_numpy(d["actions"][idx])
    r, dn = _t64(d["rewards"][idx]), _t64(d["dones"][idx])
    ar = torch.arange(B)
    q = _net(online, s)
    qa = q[ar, a]
    with torch.no_grad():
        qt = _net(target, sn)
        if v["double_dqn"]:
            boot = _net(online, sn).argmax(dim=1)
        elif v["mask"]:
            m = torch.from_numpy(d["mask"]) > 0.5
            boot = torch.zeros(B, dtype=torch.long)
            for b in range(B):                                     # first maximum over the allowed actions, else action 0
                allowed = [j for j in range(A) if m[b, j]]
                if allowed:
                    boot[b] = max(allowed, key=lambda j: (float(qt[b, j]), -j))
        else:
            boot = qt.argmax(dim=1)
        y = r + Q.GAMMA * qt[ar, boot] * (1.0 - dn)
    w = torch.ones(B, dtype=torch.float64)
    if v["is_w"]:
        w = w * _t64(d["is_w"])
    if v["w_uniform"]:
        w = w * float(d["w_uniform"])
    td = torch.zeros((), dtype=torch.float64) if v["td_off"] else (w * (qa - y) ** 2).mean()
    pen = (torch.logsumexp(q, dim=1) - math.log(A) - qa).mean()
    loss = td + v["alpha"] * pen
    grads = torch.autograd.grad(loss, online, allow_unused=True)
    grads = [np.zeros(p.shape) if g is None else g.numpy() for g, p in zip(grads, online)]
    td_abs = np.zeros(B) if v["td_off"] else (qa - y).abs().detach().numpy()
    return dict(stats=np.array([float(loss.detach()), float(td.detach()), float(pen.detach())]), grads=grads, td_abs=td_abs, boot=boot.numpy())


@pytest.mark.parametrize("name", NAMES)
def test_step64_matches_float64_autograd(name):
    d, ref, _ = _made(name)
    want = _autograd(d)
    np.testing.assert_array_equal(ref["boot"], want["boot"])
    np.testing.assert_allclose(ref["stats"], want["stats"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(ref["td_abs"], want["td_abs"], rtol=1e-10, atol=1e-14)
    for l, (g, w) in enumerate(zip(ref["grads"], want["grads"])):
        assert g.shape == w.shape
        np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-12 * Q.grad_scale(w), err_msg=f"tensor {l}")


def test_adam64_matches_torch_adam():
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal((7, 5))
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=Q.LR, betas=Q.BETAS, eps=Q.EPS)
    mine, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 4):
        g = rng.standard_normal(p0.shape) * 10.0 ** rng.integers(-4, 1, p0.shape)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        mine, m, v = Q.adam64(mine, g, m, v, step=step)
        st = opt.state[p]
        np.testing.assert_allclose(mine, p.detach().numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-20)


@pytest.mark.parametrize("name", NAMES)
def test_case_margins(name):
    d, ref, _ = _made(name)
    case, v = d["case"], Q.variant(d["case"])
    B, A, idx = case["B"], case["A"], d["idx"]
    assert d["n_rows"] == 3 * B + 7 and d["n_decided"] >= B
    assert idx.shape == (B,) and len(set(idx.tolist())) == B and idx.min() >= 0 and idx.max() < d["n_rows"]
    # every row of the batch is decided, recomputed here from the definitions
    xs, xn = d["states"][idx], d["next_states"][idx]
    _, _, zs = Q._forward(d["online"], xs, np.float64)
    assert min(float(np.abs(z).min()) for z in zs) >= Q.MARGIN
    qo = Q._forward(d["online"], xn, np.float64)[0]
    gap = Q._top2_gap(qo)
    assert ((gap >= Q.MARGIN) | d["tie_rows"]).all()
    if B > 1:
        assert (np.diff(idx) < 0).any()                                         # non-monotone
    if B >= 17:
        assert set(np.unique(d["dones"][idx])) == {0.0, 1.0}
    assert set(np.unique(d["dones"])) <= {0.0, 1.0}
    if d["n_rows"] >= 50:
        assert 0.1 < d["dones"].mean() < 0.45                                   # about a quarter
    assert ((d["actions"] >= 0) & (d["actions"] < A)).all()
    assert d["is_w"].min() >= 0.2 and d["is_w"].max() <= 1.0 and float(d["w_uniform"]) != 1.0
    assert all((x >= 0).all() for x in d["adam_v"])
    if v["mask"] and B >= 3:
        assert (d["mask"][1] == 0).all() and (d["mask"][2] == 1).all()
        assert ref["boot"][1] == 0 and d["dones"][idx[1]] == 0
        assert np.abs(Q.td_abs_for_action(d, ref, int(ref["q_target_next"][1].argmax())) - ref["td_abs"])[1] > 1e-3
    if v["mask"]:
        assert set(np.unique(d["mask"])) <= {0.0, 1.0}
    if case["tie"]:
        j1, j2 = Q.TIE_PAIR
        q32 = Q._forward(d["online"], xn, np.float32)[0]
        live = d["tie_rows"] & (d["dones"][idx] == 0)
        assert int(live.sum()) >= 3
        for qq in (qo, q32):                                      # exact ties, in both precisions, and they are the maximum
            assert (qq[d["tie_rows"], j1] == qq[d["tie_rows"], j2]).all()
            assert (qq[d["tie_rows"]].argmax(axis=1) == j1).all()
        assert (ref["boot"][d["tie_rows"]] == j1).all()
        # td_abs tells the two picks apart on those rows
        other = Q.td_abs_for_action(d, ref, j2)
        assert np.abs(other - ref["td_abs"])[live].min() > 1e-3


def test_selector_coverage():
    """Computed from the case list: every loss-stage form, output tiling, block count and depth the kernels select by."""
    masked = {Q.loss_path(c["A"], True) for c in Q.CASES if Q.variant(c)["mask"]}
    assert masked >= {"regs1", "regs2", "regs3", "regs4", "regs6", "regs8", "loop"}
    for var in ("cql", "double_dqn", "per"):
        As = {c["A"] for c in Q.CASES if c["variant"] == var}
        assert any(a <= 32 for a in As) and any(a > 32 for a in As), var
    assert any(-(-c["B"] // 16) > 64 for c in Q.CASES)              # qnet_reduce_kernel's second trip
    assert any(Q.n_lin(c) == 5 for c in Q.CASES)
    assert any(c["B"] == 1 for c in Q.CASES)
    assert {c["variant"] for c in Q.CASES} == set(Q.VARIANTS)
    # the eight-lane mapping's edges: an A on both sides of every multiple of 8 up to 32, and of the 32-column tile
    As = {c["A"] for c in Q.CASES}
    for edge in (8, 16, 24, 32):
        assert edge in As and edge + 1 in As
    assert max(As) == 128
    assert all(c["covers"] for c in Q.CASES)


def test_fp32_control_error_is_small():
    """A bound on the INPUTS: the GPU bars are max(floor, 2 x control), so a badly conditioned case must not inflate them."""
    worst = dict(td_abs=0.0, stats=0.0, grads=0.0)
    for name in NAMES:
        _, r64, r32 = _made(name)
        np.testing.assert_array_equal(r32["boot"], r64["boot"], err_msg=name)
        e = Q.errors(r64, r32)
        for k, x in (("td_abs", e["td_abs"]), ("stats", e["stats"]), ("grads", max(e["grads"]))):
            worst[k] = max(worst[k], x)
            assert x <= 5e-6, (name, k, x)
    print("worst fp32 control error:", worst)
