"""The QR-DQN, C51 and IQN loss-head kernels (csrc/dist_losses.hpp) per row and per element against the float64 oracle
(oracle/dist_oracle.py), beyond one 64-lane wave: every `for (j = lane; j < N; j += 64)` loop runs up to four trips, rows
are padded (ld > A*N, padding filled with NaN), the last block has idle waves (B % 4 != 0), and the branches small random
networks never reach (clamp mask, exact hits, |u| == kappa, ties over more than 64 entries) are built on purpose.

Bounds.  A kernel is held to BOUND_FACTOR times the error the reference's own float32 evaluation makes against the same
oracle, worst row of the worst shape of the kernel's grid.  The factor covers the kernel's summation order (sequential
over i inside a lane, then a 6-step shuffle tree, where torch sums pairwise).  The *_REF_* constants were measured on the
CPU, never taken from a kernel:

    python tests/test_dist_oracle.py

prints them, and tests/test_dist_oracle.py::test_gpu_bounds_are_the_measured_float32_reference_error re-measures them.
Error figures (oracle/dist_cases.py: head_errors): gradient - largest |difference| in a row over the row's largest
oracle gradient entry; loss - |difference| over (|row loss| + B * that entry).

Input conditions (asserted on the oracle's diagnostics, for every row - no row is left out of any comparison): the two
best next-action values lie GAP_MIN of the value scale apart, and no taken-action probability is within a factor 2 of
the 1e-8 clamp; tests/test_dist_oracle.py checks on the CPU that every case below meets them.
"""
import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import dist_cases as D
from oracle import dist_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

BOUND_FACTOR = 4
# float32 reference against the float64 oracle, worst case over the grid; the shape is (N, A, B, kappa | support) or
# (N', N'', B, kappa).  Measured with `python tests/test_dist_oracle.py`.
QR_REF_LOSS_ERR = 2.4567649185044156e-07      # (256, 18, 257, 0.6)
QR_REF_GRAD_ERR = 5.378557499050349e-05       # (1, 3, 257, 0.6): u = T - theta cancels in the row's only entry
C51_REF_LOSS_ERR = 1.1237599144806814e-05     # (51, 18, 257, (-10.0, 10.0))
C51_REF_GRAD_ERR = 4.5428885687175896e-05     # (2, 3, 257, (0.0, 200.0))
IQN_REF_LOSS_ERR = 2.2867129317960685e-07     # (65, 128, 257, 0.6)
IQN_REF_GRAD_ERR = 1.7045603690121334e-05     # (1, 11, 257, 1.0)
QR_BOUNDS = (BOUND_FACTOR * QR_REF_LOSS_ERR, BOUND_FACTOR * QR_REF_GRAD_ERR)
C51_BOUNDS = (BOUND_FACTOR * C51_REF_LOSS_ERR, BOUND_FACTOR * C51_REF_GRAD_ERR)
IQN_BOUNDS = (BOUND_FACTOR * IQN_REF_LOSS_ERR, BOUND_FACTOR * IQN_REF_GRAD_ERR)

SENTINEL = 7.0


def _N():
    from porl_amd import _native
    return _native


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _padded(a, ld):
    """(B, A, N) host array -> (B, ld) device rows; the padding columns hold NaN, so a read of them shows."""
    B = a.shape[0]
    t = torch.full((B, ld), float("nan"), dtype=torch.float32)
    t[:, :a[0].size] = torch.from_numpy(a.reshape(B, -1))
    return t.to(DEV)


class _Guarded:
    """dz (B, ld) and row_loss (B,) with one sentinel row before and after each; the output rows themselves start as
    sentinels too, so an element the kernel does not write shows."""

    def __init__(self, B, ld):
        self.B = B
        self.dz_all = torch.full((B + 2, ld), SENTINEL, dtype=torch.float32, device=DEV)
        self.rl_all = torch.full((B + 2,), SENTINEL, dtype=torch.float32, device=DEV)
        self.dz, self.rl = self.dz_all[1:B + 1], self.rl_all[1:B + 1]

    def read(self):
        dz, rl = self.dz_all.cpu().numpy(), self.rl_all.cpu().numpy()
        assert (dz[0] == SENTINEL).all() and (dz[-1] == SENTINEL).all(), "a gradient row outside the batch was written"
        assert rl[0] == SENTINEL and rl[-1] == SENTINEL, "a loss term outside the batch was written"
        return rl[1:-1], dz[1:-1]


def _qr(c, gamma, kappa, pad=0, n_quantiles=None):
    """porl_qr_loss on the case; returns (rc, row_loss, dz (B, ld))."""
    N = _N()
    B, A, NQ = c["z_cur"].shape
    ld = A * NQ + pad
    zc, zo, zt = (_padded(c[k], ld) for k in ("z_cur", "z_next_online", "z_next_target"))
    act, rew, done = _dev(c["actions"]), _dev(c["rew"]), _dev(c["done"])
    out = _Guarded(B, ld)
    rc = N.lib().porl_qr_loss(N.ptr(zc), N.ptr(zo), N.ptr(zt), ld, N.ptr(act), N.ptr(rew), N.ptr(done), B, A,
                              NQ if n_quantiles is None else n_quantiles, gamma, kappa, N.ptr(out.dz), N.ptr(out.rl),
                              N.current_stream_ptr(zc))
    return (rc,) + out.read()


def _c51(c, gamma, pad=0, n_atoms=None):
    N = _N()
    B, A, NA = c["logits_cur"].shape
    ld = A * NA + pad
    lc, lt = _padded(c["logits_cur"], ld), _padded(c["logits_next_target"], ld)
    act, rew, done, sup = _dev(c["actions"]), _dev(c["rew"]), _dev(c["done"]), _dev(c["support"])
    out = _Guarded(B, ld)
    rc = N.lib().porl_c51_loss(N.ptr(lc), N.ptr(lt), ld, N.ptr(act), N.ptr(rew), N.ptr(done), N.ptr(sup), B, A,
                               NA if n_atoms is None else n_atoms, gamma, float(c["v_min"]), float(c["v_max"]), N.ptr(out.dz),
                               N.ptr(out.rl), N.current_stream_ptr(lc))
    return (rc,) + out.read()


def _iqn(c, kappa):
    N = _N()
    B, Np = c["cur"].shape
    cur, tgt, taus = _dev(c["cur"]), _dev(c["target"]), _dev(c["taus"])
    out = _Guarded(B, Np)
    rc = N.lib().porl_iqn_quantile_huber(N.ptr(cur), N.ptr(tgt), N.ptr(taus), B, Np, c["target"].shape[1], kappa, N.ptr(out.dz),
                                         N.ptr(out.rl), N.current_stream_ptr(cur))
    return (rc,) + out.read()


def _check(what, got, o, actions, A, N, bounds):
    """Kernel output of one case against the oracle result `o`: every row, every element."""
    rc, rl, dz = got
    assert rc == 0, what
    B = len(rl)
    assert np.isfinite(rl).all() and np.isfinite(dz).all(), f"{what}: a padding column or an unwritten element shows"
    d = dz[:, :A * N].reshape(B, A, N)
    if actions is not None:
        outside = np.ones((B, A, N), bool)
        outside[np.arange(B), actions] = False
        assert not d[outside].any(), f"{what}: gradient outside the taken action's block"
        assert not dz[:, A * N:].any(), f"{what}: gradient in the padding columns"
    loss_err, grad_err = D.head_errors(rl, d, o)
    print(f"{what}: loss error {loss_err:.3g} (bound {bounds[0]:.3g}), gradient error {grad_err:.3g} (bound {bounds[1]:.3g})")
    assert loss_err <= bounds[0], f"{what}: loss error {loss_err} > {bounds[0]}"
    assert grad_err <= bounds[1], f"{what}: gradient error {grad_err} > {bounds[1]}"


# -- QR-DQN -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", D.QR_N)
def test_qr_head_equals_the_oracle_over_the_grid(N):
    for A in D.GRID_A:
        for B in D.GRID_B:
            c = D.qr_case(N, A, B)
            for kappa in D.QR_KAPPA:
                _, o = D.oracle_of("qr", (N, A, B, kappa), c)
                assert D.gap_ok(o).all()
                for pad in D.GRID_LD_PAD:
                    _check(f"qr N={N} A={A} B={B} kappa={kappa} ld=A*N+{pad}", _qr(c, D.GAMMA, kappa, pad), o, c["actions"], A, N,
                           QR_BOUNDS)


@pytest.mark.parametrize("name", ["done_all", "gamma_zero", "integers_n4", "integers_n64", "tie_n200"])
def test_qr_head_edge_cases(name):
    c, gamma, kappa, exact = D.qr_edge_cases()[name]
    o = D.qr_oracle(c, gamma, kappa)
    B, A, N = c["z_cur"].shape
    if name == "tie_n200":
        # two action means tie exactly over 200 entries: the first maximum wins; which of the two target rows was used shows
        # in the whole gradient row, and the wrong one is far outside the bound
        assert (o["gap"] == 0).all()
        np.testing.assert_array_equal(o["next_action"], c["tie_first"])
    else:
        assert D.gap_ok(o).all()
    for pad in D.GRID_LD_PAD:
        got = _qr(c, gamma, kappa, pad)
        _check(f"qr {name} ld=A*N+{pad}", got, o, c["actions"], A, N, QR_BOUNDS)
        if exact:
            # integers, gamma = kappa = 1, dyadic tau: |u| == kappa and u == 0 occur, every product and sum is exact in float32,
            # so the kernel's numbers are the oracle's, bit for bit - both Huber branches and the u < 0 indicator included
            np.testing.assert_array_equal(got[1].astype(np.float64), o["row_loss"])
            np.testing.assert_array_equal(got[2][:, :A * N].reshape(B, A, N).astype(np.float64), o["grad"])


@pytest.mark.parametrize("head", ["qr", "c51"])
def test_more_than_256_entries_per_action_is_an_error_and_writes_nothing(head):
    """N = 257 is past the kernels' 256-entry LDS rows: the entry point refuses it and leaves both outputs alone (_Guarded
    starts them as sentinels; the case is laid out for 257 entries, so nothing would be out of bounds either way)."""
    if head == "qr":
        rc, rl, dz = _qr(D.qr_case(257, 3, 5), D.GAMMA, 1.0)
    else:
        rc, rl, dz = _c51(D.c51_case(257, 3, 5, (-10.0, 10.0)), D.GAMMA)
    assert rc != 0
    assert b"N <= 256" in _N().lib().porl_last_error()
    assert (rl == SENTINEL).all() and (dz == SENTINEL).all()


# -- C51 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("support", D.C51_SUPPORT)
@pytest.mark.parametrize("N", D.C51_N)
def test_c51_head_equals_the_oracle_over_the_grid(N, support):
    for A in D.GRID_A:
        for B in D.GRID_B:
            c, o = D.oracle_of("c51", (N, A, B, support))
            assert D.gap_ok(o).all() and D.clamp_ok(o).all()
            for pad in D.GRID_LD_PAD:
                _check(f"c51 N={N} A={A} B={B} support={support} ld=A*N+{pad}", _c51(c, D.GAMMA, pad), o, c["actions"], A, N,
                       C51_BOUNDS)


@pytest.mark.parametrize("name", sorted(D.c51_edge_cases()))
def test_c51_head_edge_cases(name):
    c = D.c51_edge_cases()[name]
    o = D.c51_oracle(c, c["gamma"])
    assert D.gap_ok(o).all() and D.clamp_ok(o).all()
    B, A, N = c["logits_cur"].shape
    rows = np.arange(B)
    for pad in D.GRID_LD_PAD:
        got = _c51(c, c["gamma"], pad)
        _check(f"c51 {name} ld=A*N+{pad}", got, o, c["actions"], A, N, C51_BOUNDS)
        if c.get("uniform_cur"):
            # zero online logits: p = 1/N and the clamp mask is one everywhere, so dl_k = -(m_k - 1/N) / B and the projected
            # distribution is read back atom by atom - mass on the wrong atom shows here, not in a sum
            m = 1.0 / N - B * got[2][:, :A * N].reshape(B, A, N)[rows, c["actions"]].astype(np.float64)
            err = np.abs(m - o["m"]).max(axis=1) / np.abs(o["m"] - 1.0 / N).max(axis=1)
            print(f"c51 {name}: projected distribution, worst atom {err.max():.3g}")
            assert err.max() <= C51_BOUNDS[1]
            if c.get("one_atom"):
                np.testing.assert_array_equal(m.argmax(axis=1), o["m"].argmax(axis=1))
                assert (np.sort(m, axis=1)[:, -2] <= C51_BOUNDS[1]).all()


# -- IQN --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Npp", D.IQN_NPP)
@pytest.mark.parametrize("Np", D.IQN_NP)
def test_iqn_head_equals_the_oracle_over_the_grid(Np, Npp):
    for B in D.GRID_B:
        c = D.iqn_case(Np, Npp, B)
        for kappa in D.IQN_KAPPA:
            _, o = D.oracle_of("iqn", (Np, Npp, B, kappa), c)
            _check(f"iqn N'={Np} N''={Npp} B={B} kappa={kappa}", _iqn(c, kappa), o, None, 1, Np, IQN_BOUNDS)


# -- the reference's own numbers ----------------------------------------------------------------------------------------------
# kernel and golden are two float32 evaluations: the kernel within BOUND_FACTOR * REF of the oracle, the reference within REF
GOLDEN_FACTOR = BOUND_FACTOR + 1


@pytest.mark.parametrize("name", ["qr_head_n51", "qr_head_n200", "c51_head_n51", "c51_head_n101"])
def test_heads_reproduce_the_reference_golden(name):
    z = dict(np.load(__import__("os").path.join(GOLDEN, name + ".npz")))
    if name.startswith("qr"):
        o = D.qr_oracle(z, float(z["gamma"]), float(z["kappa"]))
        key, ref_loss, ref_grad = "z_cur", QR_REF_LOSS_ERR, QR_REF_GRAD_ERR
        got = _qr(z, float(z["gamma"]), float(z["kappa"]), pad=3)
    else:
        o = D.c51_oracle(z, float(z["gamma"]))
        assert D.clamp_ok(o).all()
        key, ref_loss, ref_grad = "logits_cur", C51_REF_LOSS_ERR, C51_REF_GRAD_ERR
        got = _c51(z, float(z["gamma"]), pad=3)
    assert D.gap_ok(o).all()
    B, A, N = z[key].shape
    _check(name, got, o, z["actions"], A, N, (BOUND_FACTOR * ref_loss, BOUND_FACTOR * ref_grad))
    rc, rl, dz = got
    loss = float(rl.astype(np.float64).mean())
    gmax = np.abs(z["grad"]).reshape(B, -1).max(axis=1)
    assert abs(loss - float(z["loss"])) <= GOLDEN_FACTOR * ref_loss * (abs(float(z["loss"])) + B * gmax.mean())
    d = dz[:, :A * N].reshape(B, A, N)
    assert (np.abs(d - z["grad"]).reshape(B, -1).max(axis=1) <= GOLDEN_FACTOR * ref_grad * gmax).all()


# -- one learn() of the trainers at their class defaults ------------------------------------------------------------------------
def _load_pairs(module, layers):
    keys = list(module.state_dict().keys())
    assert len(keys) == 2 * len(layers)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in zip(keys, [a for pair in layers for a in pair])})
    return keys


def _make_trainer(spec, **kw):
    from porl_amd.train.c51_trainer import C51Trainer
    from porl_amd.train.qr_dqn_trainer import QRDQNTrainer
    if spec["kind"] == "qr":
        t = QRDQNTrainer(spec["S"], spec["A"], spec.get("gamma", 0.99), device=DEV, num_quantiles=spec["N"], **kw)
        assert spec["N"] != 51 or (t.num_quantiles, t.kappa) == (51, 1.0)
    else:
        t = C51Trainer(spec["S"], spec["A"], spec.get("gamma", 0.99), device=DEV, atom_size=spec["N"], **kw)
        assert (t.v_min, t.v_max) == (-10, 10)
    assert t.q_network._spec[2] == [128, 128] and t.batch_size == 64
    return t


@pytest.mark.parametrize("name", sorted(D.TRAINER_CASES))
def test_trainer_step_at_class_defaults_equals_the_oracle(name):
    """One learn_on at the class defaults (hidden [128, 128], 51 quantiles / atoms, C51 on [-10, 10]; `qr_n200_a5`: 200
    quantiles on 5 actions, a 1000-wide output layer through the grouped GEMM) against the oracle head on float64 forward
    passes.  Loss: rtol 2e-5, the bound tests/test_cql_gpu.py holds the same engine path to (three float32 GEMM layers of
    K <= 128 in front of a loss that is Lipschitz in the outputs).  First Adam step of the output-layer bias: with zero
    moments the step is -lr * g / (|g| + eps) exactly, so wherever |g| > 1e-6 (float32 rounding of g is ~1e-9 there) the
    sign is the oracle's and the size follows that formula to 1e-3."""
    spec = D.TRAINER_CASES[name]
    c, o, gb = D.trainer_case(spec)
    assert D.gap_ok(o).all() and (spec["kind"] == "qr" or D.clamp_ok(o).all())
    t = _make_trainer(spec)
    keys = _load_pairs(t.q_network, c["online"])
    _load_pairs(t.target_network, c["target"])
    before = t.q_network.state_dict()[keys[-1]].cpu().double().numpy().copy()
    loss = t.learn_on(*(_dev(c[k]) for k in ("states", "actions", "rew", "next_states", "done")))
    want = float(o["row_loss"].mean())
    print(f"{name}: loss {loss!r}, oracle {want!r}")
    np.testing.assert_allclose(loss, want, rtol=2e-5)
    moved = t.q_network.state_dict()[keys[-1]].cpu().double().numpy() - before
    big = np.abs(gb) > 1e-6
    assert big.sum() > 100
    np.testing.assert_array_equal(np.sign(moved[big]), -np.sign(gb[big]))
    lr, eps = t.optimizer.param_groups[0]["lr"], t.optimizer.param_groups[0]["eps"]
    np.testing.assert_allclose(np.abs(moved[big]), lr * np.abs(gb[big]) / (np.abs(gb[big]) + eps), rtol=1e-3)
    assert not moved[~big & (gb == 0)].any()                     # columns of actions nobody took: no gradient, no step


def test_qr_trainer_with_300_quantiles_raises():
    """300 quantiles are past the loss head's 256: the native call refuses, and the trainer passes that on."""
    from porl_amd._native import NativeError
    spec = dict(D.TRAINER_CASES["qr_default"], N=300)
    c = D.mlp_case(spec["S"], spec["A"] * 300, spec["hidden"], spec["B"], spec["A"], seed=0)
    t = _make_trainer(spec)
    with pytest.raises(NativeError, match="N <= 256"):
        t.learn_on(*(_dev(c[k]) for k in ("states", "actions", "rew", "next_states", "done")))


# -- greedy-action epilogue of the act kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(D.ACT_CASES))
def test_act_epilogue_equals_the_oracle_argmax(name):
    """porl_qnet_act kinds 1 (C51 expectation) and 2 (QR mean) with n_sub = 51 and with A * n_sub = 1000, batches of 1 and 8
    from rows of a device array: the greedy action is the float64 argmax on every row (all rows meet the gap condition)."""
    spec = D.ACT_CASES[name]
    c, best, gap, scale = D.act_case(spec)
    assert (gap >= D.GAP_MIN * scale).all()
    t = _make_trainer(dict(spec, gamma=0.99))
    _load_pairs(t.q_network, c["online"])
    kind, n_sub, support = t._act_epilogue()
    assert (kind, n_sub) == (2 if spec["kind"] == "qr" else 1, spec["N"]) and spec["A"] * n_sub in (204, 1000)
    if support is not None:
        np.testing.assert_array_equal(support.cpu().numpy(), c["support"])
    eng = t._engine
    assert eng.act_ok
    rows = _dev(c["states"])
    for B in (1, 8):
        for r0 in (0, 4):
            rec = torch.full((16,), -1, dtype=torch.int32).pin_memory()
            eng.act(rec, states=rows, row=r0, batch=B, kind=kind, n_act=spec["A"], n_sub=n_sub, support=support)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(rec[:B].numpy(), best[r0:r0 + B], err_msg=f"{name} batch {B} from row {r0}")
