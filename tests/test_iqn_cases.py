"""CPU checks of the engine cases in tests/helpers/iqn_cases.py, the yardstick of tests/test_iqn_engine_gpu.py: the oracle's
fp64 step (oracle/iqn_oracle.IqnOracle, started from given Adam moments and a step number) against torch autograd in
float64 on a plain restatement of the network and loss, adam64 against torch.optim.Adam, the margins of every learn case
(a minibatch full of decided samples: the GPU comparison leaves none out) and of every act state, the coverage of the
kernels' branches computed from the case lists, and the fp32 control's own error, which sets the GPU bars."""
import functools

import numpy as np
import pytest
import torch

from helpers import iqn_cases as IC
from oracle import iqn_oracle as IO


@functools.lru_cache(maxsize=None)
def _made(name):
    d = IC.make_learn(IC.LEARN_CASES[name])
    return d, IC.step64(d), IC.step32(d)


@functools.lru_cache(maxsize=None)
def _act(kind, *key):
    return IC.act_grid_case(*key) if kind == "grid" else IC.act_probe_case(*key)


def _t64(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


def _net(P, s, taus):
    """IQNNetwork.forward, written out: (B, N, A)."""
    E = P["quantile_embedding.weight"].shape[1]
    lin = lambda x, name: x @ P[name + ".weight"].T + P[name + ".bias"]
    feat = torch.relu(lin(torch.relu(lin(s, "feature_net.0")), "feature_net.2"))
    i = torch.arange(1, E + 1, dtype=torch.float64)
    emb = lin(torch.cos(torch.pi * i * taus[..., None]), "quantile_embedding")
    return lin(torch.relu(lin(feat[:, None, :] * emb, "value_net.0")), "value_net.2")


def _autograd(d):
    """IQNTrainer.learn's loss, clip_grad_norm_ and torch.optim.Adam in float64 on the CPU."""
    c, idx = d["case"], d["idx"]
    B = c["B"]
    P = {k: _t64(v).requires_grad_(True) for k, v in d["online"].items()}
    T = {k: _t64(v) for k, v in d["target"].items()}
    s, sn = _t64(d["states"][idx]), _t64(d["next_states"][idx])
    r, dn = _t64(d["rewards"][idx]), _t64(d["dones"][idx])
    a = torch.from_numpy(d["actions"][idx])
    tp, tpp = _t64(d["taus_prime"]), _t64(d["taus_dprime"])
    ar = torch.arange(B)
    cur = _net(P, s, tp)[ar, :, a]                                                  # (B, N')
    with torch.no_grad():
        a_star = _net(P, sn, tpp).mean(dim=1).argmax(dim=1)
        td = r[:, None] + IC.GAMMA * _net(T, sn, tpp)[ar, :, a_star] * (1.0 - dn[:, None])
    u = td[:, None, :] - cur[:, :, None]
    k = c["kappa"]
    hub = torch.where(u.abs() <= k, 0.5 * u * u, k * (u.abs() - 0.5 * k))
    w = (tp[:, :, None] - (u.detach() < 0).double()).abs()
    loss = (w * hub).mean(dim=2).mean(dim=1).mean()
    params = [P[n] for n in IO.NAMES]
    for p, g in zip(params, torch.autograd.grad(loss, params)):
        p.grad = g
    opt = torch.optim.Adam(params, lr=IC.LR, betas=IC.BETAS, eps=IC.EPS)
    for n, p in zip(IO.NAMES, params):
        opt.state[p] = dict(step=torch.tensor(float(IC.STEP - 1)), exp_avg=_t64(d["adam_m"][n]).clone(),
                            exp_avg_sq=_t64(d["adam_v"][n]).clone())
    total = float(torch.nn.utils.clip_grad_norm_(params, d["max_norm"]))
    grads = [p.grad.numpy().copy() for p in params]
    opt.step()
    return dict(loss=float(loss.detach()), norm=total, grads=grads, a_star=a_star.numpy(),
                params=[p.detach().numpy() for p in params])


@pytest.mark.parametrize("name", IC.LEARN_NAMES)
def test_step64_matches_float64_autograd(name):
    d, ref, _ = _made(name)
    want = _autograd(d)
    np.testing.assert_array_equal(ref["a_star"], want["a_star"])
    np.testing.assert_allclose(ref["loss"], want["loss"], rtol=1e-10)
    np.testing.assert_allclose(ref["norm"], want["norm"], rtol=1e-10)
    for n, g, w, p, wp in zip(IO.NAMES, ref["grads"], want["grads"], ref["params"], want["params"]):
        assert g.shape == w.shape
        np.testing.assert_allclose(g, w, rtol=1e-9, atol=1e-12 * IC.grad_scale(w), err_msg=n)
        np.testing.assert_allclose(p, wp, rtol=1e-9, atol=1e-12, err_msg=n)


def test_adam64_matches_torch_adam_and_the_oracle():
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal((7, 5))
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=IC.LR, betas=IC.BETAS, eps=IC.EPS)
    mine, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 4):
        g = rng.standard_normal(p0.shape) * 10.0 ** rng.integers(-4, 1, p0.shape)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        mine, m, v = IC.adam64(mine, g, m, v, step=step)
        st = opt.state[p]
        np.testing.assert_allclose(mine, p.detach().numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-20)
    d, ref, _ = _made("ragged-a5-k1.0-clip")                # ... and the oracle's own Adam stage from the case's moments
    for i, n in enumerate(IO.NAMES):
        pp, mm, vv = IC.adam64(d["online"][n], ref["grads"][i], d["adam_m"][n], d["adam_v"][n])
        for got, want in ((ref["params"][i], pp), (ref["adam_m"][i], mm), (ref["adam_v"][i], vv)):
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-18, err_msg=n)


@pytest.mark.parametrize("name", IC.LEARN_NAMES)
def test_learn_case_is_full_of_decided_samples(name):
    d, ref, r32 = _made(name)
    c, idx = d["case"], d["idx"]
    B, A = c["B"], c["A"]
    assert d["n_rows"] == 3 * B + 7 > B
    assert idx.shape == (B,) and idx.dtype == np.int64 and len(set(idx.tolist())) == B and 0 <= idx.min() and idx.max() < d["n_rows"]
    assert d["taus_prime"].shape == (B, c["NP"]) and d["taus_dprime"].shape == (B, c["NPP"])
    assert d["taus_prime"].dtype == d["taus_dprime"].dtype == np.float32
    # every sample is decided, recomputed here on the whole minibatch
    relu, gap, tie = IC.sample_margins(c, d["online"], d["states"][idx], d["next_states"][idx], d["taus_prime"], d["taus_dprime"])
    assert relu.min() >= IC.MARGIN
    assert ((gap >= IC.MARGIN) | tie).all() and (tie == d["tie_samples"]).all()
    assert not tie.any() or c["tie"]
    # the minibatch is neither sorted nor a prefix of the replay arrays, and mixes terminal rows in
    assert (np.sort(idx) != np.arange(B)).any()
    if B > 1:
        assert (np.diff(idx) < 0).any()
    if B >= 3:
        assert set(np.unique(d["dones"][idx])) == {0.0, 1.0}
    assert set(np.unique(d["dones"])) <= {0.0, 1.0}
    assert ((d["actions"] >= 0) & (d["actions"] < A)).all()
    # a run in progress: non-zero moments, a step number above 1, a target that is not the online network
    assert IC.STEP > 1 and all(np.abs(m).min() > 0 for m in d["adam_m"].values()) and all((v > 0).all() for v in d["adam_v"].values())
    assert all((d["target"][k] != d["online"][k]).all() for k in IO.NAMES)
    # clipping: active means the fp64 norm is more than twice max_norm
    if c["clip"]:
        assert ref["norm"] > 2.0 * d["max_norm"] and ref["coef"] < 0.5
    else:
        assert ref["coef"] == 1.0 and ref["norm"] < d["max_norm"]
    assert all(np.abs(g).max() > 0 for g in ref["grads"])
    np.testing.assert_array_equal(r32["a_star"], ref["a_star"])
    if c["tie"]:
        j1, j2 = IC.TIE_PAIR
        live = tie & (d["dones"][idx] == 0)
        assert int(live.sum()) >= 3
        assert (ref["a_star"][tie] == j1).all()                                    # the first maximum
        P32 = {k: v.astype(np.float32) for k, v in d["online"].items()}
        q32 = IO.forward(P32, d["next_states"][idx], d["taus_dprime"]).mean(1)
        assert (q32[tie, j1] == q32[tie, j2]).all() and (q32[tie].argmax(1) == j1).all()
        # the other pick changes the loss by far more than any bar: the target network tells the pair apart
        T = {k: v.astype(np.float64) for k, v in d["target"].items()}
        zt = IO.forward(T, d["next_states"][idx].astype(np.float64), d["taus_dprime"].astype(np.float64))
        assert np.abs(zt[live][:, :, j1] - zt[live][:, :, j2]).mean() > 1e-2


ACT_IDS = [("grid",) + k for k in IC.ACT_GRID] + [("probe",) + k for k in IC.ACT_PROBES]


@pytest.mark.parametrize("key", ACT_IDS, ids=lambda k: "-".join(map(str, k)))
def test_every_act_state_is_decided(key):
    c = _act(*key)
    n_tau = key[2] if key[0] == "grid" else key[3]
    assert c["states"].shape == (IC.ACT2_STATES, IC.ACT2_S) and c["taus"].shape == (IC.ACT2_STATES, n_tau)
    q = IC.mean_q(c["T"] if c["which"] else c["P"], c["states"], c["taus"])
    if key[0] == "grid":
        assert (IC.top2_gap(q) >= IC.ACT_MIN_GAP).all()
        np.testing.assert_array_equal(q.argmax(1), c["want"])
        assert len(set(c["want"].tolist())) >= min(key[3], 8)
        return
    probe, H = key[1], key[2]
    if probe == "lastk":
        W, b = c["P"]["value_net.2.weight"], c["P"]["value_net.2.bias"]
        assert not W[:, :H - 1].any() and W[:, H - 1].all()
        assert (IC.top2_gap(q) >= IC.ACT_MIN_GAP).all() and (c["want"] == q.argmax(1)).all()
        assert (c["want"] != int(np.argmax(b))).all()        # a head that misses k = H - 1 answers with its largest bias
    elif probe in ("nan1", "nan2"):
        where = (2,) if probe == "nan1" else (1, 3)
        assert np.isnan(q[:, where]).all() and np.isfinite(np.delete(q, where, axis=1)).all()
        np.testing.assert_array_equal(q.argmax(1), c["want"])                      # numpy's argmax has torch's NaN rule
        np.testing.assert_array_equal(torch.from_numpy(q).argmax(dim=1).numpy(), c["want"])
        assert (c["want"] == where[0]).all()
        finite = np.where(np.isnan(q), -np.inf, q)
        assert (finite.argmax(1) != where[0]).any()          # a plain `>` would answer otherwise
    else:
        qo = IC.mean_q(c["P"], c["states"], c["taus"])
        assert (IC.top2_gap(q) >= IC.ACT_MIN_GAP).all() and (IC.top2_gap(qo) >= IC.ACT_MIN_GAP).all()
        assert (q.argmax(1) == c["want"]).all() and (qo.argmax(1) != c["want"]).all()


def test_branch_coverage():
    """Computed from the case lists with selectors that mirror the kernels' conditions."""
    L = list(IC.LEARN_CASES.values())
    rows = lambda c: c["B"] * c["NP"]
    assert any(c["B"] == 1 for c in L)
    # Hp > H with unaligned parameter rows, and Hp == H; Ap > A and Ap == A
    assert any(IC.ru4(c["H"]) > c["H"] and c["H"] % 4 == 2 for c in L) and any(IC.ru4(c["H"]) == c["H"] for c in L)
    assert any(IC.ru4(c["A"]) > c["A"] for c in L) and any(IC.ru4(c["A"]) == c["A"] for c in L)
    # padding in the flat buffers
    assert any(any(int(np.prod(s)) % 4 for s in IC.shapes_of(c["S"], c["H"], c["E"], c["A"])) for c in L)
    # embedding wgrad: a second staging trip with a partial (one-row) tile; one-column last blocks in H and in E
    assert any(IC.sel_wgrad_trips(rows(c)) == (2, 1) for c in L) and any(IC.sel_wgrad_trips(rows(c))[0] == 1 for c in L)
    assert any(IC.sel_last_block(c["H"], IC.WG_T) == 1 and c["H"] > IC.WG_T for c in L)
    assert any(IC.sel_last_block(c["E"], IC.WG_T) == 1 and c["E"] > IC.WG_T for c in L)
    # mix: a one-row fifth tile, a one-column second column block, the k < E tail, the full panels
    assert any(IC.sel_mix_tiles(rows(c)) == (5, 1) for c in L)
    assert any(IC.sel_last_block(c["H"], IC.MIX_COLS) == 1 and c["H"] > IC.MIX_COLS for c in L)
    assert any(c["E"] % 8 for c in L) and any(c["E"] == IC.MAX_E for c in L) and any(c["E"] == 1 for c in L)
    # head: passes of the Bellman-target loop and of the loss loop; the limits
    assert {IC.sel_lane_passes(c["NPP"]) for c in L} >= {1, 4} and {IC.sel_lane_passes(c["NP"]) for c in L} >= {1, 2}
    assert any(c["NPP"] == IC.MAX_TAU for c in L) and any(c["A"] == IC.MAX_A for c in L)
    ragged = {(c["A"], c["kappa"]) for c in L if c["shape"] == "ragged" and not c["clip"] and not c["tie"]}
    assert ragged >= {(a, k) for a in IC.RAGGED_ACTIONS for k in IC.KAPPAS}
    for s in IC.LEARN_SHAPES:
        assert {c["clip"] for c in L if c["shape"] == s} == {False, True}
    assert sum(c["tie"] for c in L) == 1 and all(c["covers"] for c in L)
    # act: both branches of the head's loads, both thread counts on either side of 16, the LDS corner, the action tail
    G = IC.ACT_GRID
    assert {IC.sel_vec(H) for H, _, _ in G} == {False, True}
    assert {(n, IC.sel_act_threads(n)) for _, n, _ in G} >= {(15, 256), (16, 1024), (17, 1024), (1, 256), (256, 1024)}
    assert all((H, IC.MAX_TAU, IC.MAX_A) in G for H in (30, 32))
    assert {A % 4 for _, _, A in G} >= {0, 1} and {A for _, _, A in G} >= {1, 5, 64}
    P = IC.ACT_PROBES
    for probe in ("lastk", "nan1", "nan2", "target"):
        assert {(IC.sel_vec(H), IC.sel_act_threads(n)) for p, H, n in P if p == probe} == {(v, t) for v in (False, True) for t in (256, 1024)}


def test_fp32_control_error():
    """The control's worst error per quantity: the GPU bars are max(2e-6, 2 x control), so this is what a badly conditioned
    case would inflate.  Printed, and held below a cap so that no case can buy itself a wide bar: 1e-5 (fp32's unit
    roundoff, 6e-8, times the ~100 operations a value passes through), or, where it is more, the error fp32 leaves in the
    widest cosine feature: the argument (fl32(pi) * E) * tau <= pi * E is rounded twice, 2 x 2^-24 x pi x E, which
    cos passes on to a feature of order one (4.8e-5 at E = 128)."""
    worst = {}
    for name in IC.LEARN_NAMES:
        d, r64, r32 = _made(name)
        cap = max(1e-5, 2.0 * 2.0 ** -24 * np.pi * d["case"]["E"])
        e = IC.learn_errors(r64, r32)
        for k, x in [(k, e[k]) for k in IC.STAT_NAMES] + [("grad " + n, x) for n, x in zip(IO.NAMES, e["grads"])]:
            if x > worst.get(k, (0.0, ""))[0]:
                worst[k] = (x, name)
            assert x <= cap, (name, k, x, cap)
    print("worst fp32 control error per quantity:")
    for k, (x, name) in worst.items():
        print(f"    {k:34s} {x:.3g}  ({name})")
