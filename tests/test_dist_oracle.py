"""The float64 oracle of the distributional loss heads (oracle/dist_oracle.py) against the reference's own numbers and
against autograd, and everything tests/test_dist_heads_gpu.py takes as given: the measured float32-reference error
behind its bounds and the input conditions of its cases.  CPU only.

    python tests/test_dist_oracle.py        prints the measured table (the constants of tests/test_dist_heads_gpu.py)
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import dist_cases as D          # noqa: E402
from oracle import dist_oracle as O         # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# oracle (float64) against numbers the reference computed in float32.  Each term of these losses is a handful of float32
# operations (relative error a few 2^-24 = 6e-8) and torch sums pairwise, so the scalar loss is good to about 1e-6
# relative; 5e-6 leaves a margin.  The gradient is held to the measured worst case of the same float32 evaluation over
# the whole GPU grid (the REF_* constants of tests/test_dist_heads_gpu.py, re-measured below): the goldens are two more
# shapes of that family.
GOLDEN_LOSS_RTOL = 5e-6


def _golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _bounds():
    import test_dist_heads_gpu as G
    return G


@pytest.mark.parametrize("name", ["qr_head_n51", "qr_head_n200"])
def test_oracle_reproduces_the_reference_qr_head(name):
    z = _golden(name)
    o = D.qr_oracle(z, float(z["gamma"]), float(z["kappa"]))
    assert D.gap_ok(o).all()
    np.testing.assert_allclose(o["row_loss"].mean(), float(z["loss"]), rtol=GOLDEN_LOSS_RTOL)
    _, ge = D.head_errors(o["row_loss"], z["grad"], o)
    print(name, "gradient error of the reference's float32 numbers:", ge)
    assert ge <= _bounds().QR_REF_GRAD_ERR
    taken = np.zeros(z["grad"].shape[:2], bool)
    taken[np.arange(len(taken)), z["actions"]] = True
    assert not z["grad"][~taken].any() and z["grad"][taken].any(axis=1).all()


@pytest.mark.parametrize("name", ["c51_head_n51", "c51_head_n101"])
def test_oracle_reproduces_the_reference_c51_head(name):
    z = _golden(name)
    o = D.c51_oracle(z, float(z["gamma"]))
    assert D.gap_ok(o).all() and D.clamp_ok(o).all()
    tz = z["rew"][:, None] + float(z["gamma"]) * z["support"][None] * (1 - z["done"][:, None])
    assert (tz < z["v_min"]).any() and (tz > z["v_max"]).any()                 # both clamps of the support occur
    np.testing.assert_allclose(o["row_loss"].mean(), float(z["loss"]), rtol=GOLDEN_LOSS_RTOL)
    _, ge = D.head_errors(o["row_loss"], z["grad"], o)
    print(name, "gradient error of the reference's float32 numbers:", ge)
    assert ge <= _bounds().C51_REF_GRAD_ERR


def test_oracle_reproduces_the_reference_iqn_head():
    z = _golden("iqn_quantile_huber")
    o = O.iqn_head(z["cur"], z["target"], z["taus"], float(z["kappa"]))
    np.testing.assert_allclose(o["row_loss"].mean(), float(z["loss"]), rtol=GOLDEN_LOSS_RTOL)
    _, ge = D.head_errors(o["row_loss"], z["dcur"], o)
    assert ge <= _bounds().IQN_REF_GRAD_ERR


# -- hand-derived gradients against autograd, both in float64 ------------------------------------------------------------
AUTOGRAD_TOL = 1e-12     # two float64 evaluations of the same sums in different orders: ~N * 1e-16 of O(1) numbers


@pytest.mark.parametrize("N,A,B,kappa", [(7, 3, 6, 0.6), (70, 5, 9, 1.0)])
def test_qr_gradient_equals_autograd(N, A, B, kappa):
    c, o = D.oracle_of("qr", (N, A, B, kappa))
    rows, grad, nxt = D.torch_qr(c, D.GAMMA, kappa, torch.float64)
    np.testing.assert_array_equal(nxt, o["next_action"])
    np.testing.assert_allclose(rows, o["row_loss"], rtol=AUTOGRAD_TOL)
    np.testing.assert_allclose(grad, o["grad"], atol=AUTOGRAD_TOL * np.abs(o["grad"]).max())


@pytest.mark.parametrize("N,A,B,support,span", [(9, 3, 6, (-10.0, 10.0), None), (70, 5, 9, (0.0, 200.0), None),
                                                (33, 3, 7, (-10.0, 10.0), 30.0)])
def test_c51_gradient_and_projection_equal_autograd(N, A, B, support, span):
    """span = 30: the rows reach below the 1e-8 clamp, so the mask c_n of the hand-derived gradient is exercised."""
    c = D.c51_case(N, A, B, support, seed="autograd", cur_span=span)
    o = D.c51_oracle(c, D.GAMMA)
    assert D.gap_ok(o).all() and D.clamp_ok(o).all()
    rows, grad, nxt, m = D.torch_c51(c, D.GAMMA, torch.float64)
    if span:
        logp = O._log_softmax(c["logits_cur"].astype(np.float64)[np.arange(B), c["actions"]])
        below = np.exp(logp) < O.CLAMP_MIN
        assert (below & (o["m"] > 1e-4)).any(axis=1).sum() >= B // 2 and (below.any(axis=1) & (~below).any(axis=1)).all()
    np.testing.assert_array_equal(nxt, o["next_action"])
    np.testing.assert_allclose(m, o["m"], atol=AUTOGRAD_TOL)
    np.testing.assert_allclose(rows, o["row_loss"], rtol=AUTOGRAD_TOL)
    np.testing.assert_allclose(grad, o["grad"], atol=AUTOGRAD_TOL * np.abs(o["grad"]).max())


@pytest.mark.parametrize("Np,Npp,B,kappa", [(5, 7, 6, 0.6), (70, 3, 9, 1.0)])
def test_iqn_gradient_equals_autograd(Np, Npp, B, kappa):
    c, o = D.oracle_of("iqn", (Np, Npp, B, kappa))
    rows, grad, _ = D.torch_iqn(c, kappa, torch.float64)
    np.testing.assert_allclose(rows, o["row_loss"], rtol=AUTOGRAD_TOL)
    np.testing.assert_allclose(grad, o["grad"], atol=AUTOGRAD_TOL * np.abs(o["grad"]).max())


def test_huber_branches_coincide_at_kappa():
    """L_kappa is C1: at |u| == kappa the quadratic and the linear branch give the same value and the same slope, in
    float32 bit for bit (0.5 * u * u and kappa * (|u| - 0.5 * kappa) are the same two roundings when |u| == kappa).  So no
    output can tell `|u| <= kappa` from `|u| < kappa`; the integer-valued GPU case pins the values at the kink instead."""
    for kappa in (np.float32(0.6), np.float32(1.0), np.float32(0.3)):
        u = kappa
        assert np.float32(0.5) * u * u == kappa * (abs(u) - np.float32(0.5) * kappa)
        L, dL = O._huber(np.array([-float(kappa), float(kappa)]), float(kappa))
        np.testing.assert_array_equal(L, 0.5 * float(kappa) ** 2)
        np.testing.assert_array_equal(dL, [-float(kappa), float(kappa)])


# -- the measured tolerance table ----------------------------------------------------------------------------------------
def measured_table():
    """{kernel: (loss error, shape, gradient error, shape)}: the float32 reference evaluation (oracle/dist_cases.py:
    torch_qr / torch_c51 / torch_iqn in torch.float32, i.e. what the reference computes) against the float64 oracle, worst
    row of the worst shape of the GPU grid.  Error figures as defined by dist_cases.head_errors."""
    return {k: D.measure_fp32_reference_error(k) for k in ("qr", "c51", "iqn")}


@pytest.mark.parametrize("kernel", ["qr", "c51", "iqn"])
def test_gpu_bounds_are_the_measured_float32_reference_error(kernel):
    """The named constants of the GPU test are this measurement, not anything a kernel produced.  A different CPU or
    thread count may reorder torch's float32 sums, which moves a worst case by a few percent; a constant further than
    a factor 1.25 from today's measurement is stale and has to be re-measured."""
    G = _bounds()
    loss_err, loss_shape, grad_err, grad_shape = D.measure_fp32_reference_error(kernel)
    print(kernel, "loss", loss_err, loss_shape, "gradient", grad_err, grad_shape)
    K = kernel.upper()
    for measured, const in ((loss_err, getattr(G, K + "_REF_LOSS_ERR")), (grad_err, getattr(G, K + "_REF_GRAD_ERR"))):
        assert const / 1.25 <= measured <= const * 1.25
    assert G.BOUND_FACTOR == 4


# -- input conditions of every GPU case -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["qr", "c51"])
def test_every_grid_row_meets_the_input_conditions(kernel):
    for shape in D.GRIDS[kernel]():
        _, o = D.oracle_of(kernel, shape)
        assert D.gap_ok(o).all(), shape
        if kernel == "c51":
            assert D.clamp_ok(o).all(), shape


def test_edge_cases_meet_the_input_conditions():
    for name, (c, gamma, kappa, exact) in D.qr_edge_cases().items():
        o = D.qr_oracle(c, gamma, kappa)
        if name == "tie_n200":
            assert (o["gap"] == 0).all()                         # the deliberate tie: exact values, first maximum
            np.testing.assert_array_equal(o["next_action"], c["tie_first"])
        else:
            assert D.gap_ok(o).all(), name
        if exact:                                                # the oracle's numbers are float32 numbers already
            assert np.array_equal(o["row_loss"], o["row_loss"].astype(np.float32)), name
            assert np.array_equal(o["grad"], o["grad"].astype(np.float32)), name
            u = o["target"][:, :, None] - c["z_cur"][np.arange(8), c["actions"]][:, None, :]
            assert (np.abs(u) == kappa).sum() > 20 and (u == 0).sum() > 10, name
    for name, c in D.c51_edge_cases().items():
        o = D.c51_oracle(c, c["gamma"])
        assert D.gap_ok(o).all() and D.clamp_ok(o).all(), name
        B = len(c["rew"])
        if c.get("identity"):
            p = np.exp(O._log_softmax(c["logits_next_target"].astype(np.float64)))[np.arange(B), o["next_action"]]
            np.testing.assert_array_equal(o["m"], p)
        if c.get("one_atom"):
            want = np.clip((c["rew"].astype(np.float64) + 10.0) / 0.5, 0, 40).astype(int)
            np.testing.assert_array_equal(o["m"].argmax(axis=1), want)
            np.testing.assert_allclose(o["m"].max(axis=1), 1.0, rtol=1e-15)
            assert ((o["m"] > 0).sum(axis=1) == 1).all()
        if c.get("clamped"):
            logp = O._log_softmax(c["logits_cur"].astype(np.float64)[np.arange(B), c["actions"]])
            below = np.exp(logp) < O.CLAMP_MIN
            assert (below & (o["m"] > 1e-4)).any(axis=1).sum() >= B // 2 and (below.any(axis=1) & (~below).any(axis=1)).all()
            assert (c["logits_cur"].max(axis=2) - c["logits_cur"].min(axis=2) == 30.0).all()


def test_trainer_and_act_cases_meet_the_input_conditions():
    for name, spec in D.TRAINER_CASES.items():
        _, o, gb = D.trainer_case(spec)
        assert D.gap_ok(o).all(), name
        if spec["kind"] == "c51":
            assert D.clamp_ok(o).all(), name
        assert len(np.unique(o["next_action"])) > 1 and (np.abs(gb) > 1e-6).sum() > 100, name
    for name, spec in D.ACT_CASES.items():
        _, best, gap, scale = D.act_case(spec)
        assert (gap >= D.GAP_MIN * scale).all() and len(np.unique(best)) > 1, name


if __name__ == "__main__":
    for k, v in measured_table().items():
        print(k, "loss error %.17g at %s; gradient error %.17g at %s" % v)
