"""Inputs, shape grids and float32 reference evaluations for the distributional loss-head tests.

TEST INFRASTRUCTURE ONLY, shared by tests/test_dist_oracle.py (CPU), tests/test_dist_heads_gpu.py and
oracle/gen_golden.py so that the shapes whose float32-reference error is measured on the CPU are exactly the shapes the
kernels are run at.

  * the grids (QR_*, C51_*, IQN_*) and seeded input builders: every random row satisfies the two input conditions under
    which a float32 and a float64 evaluation must agree (GAP_MIN of the value scale between the two best next-action
    values; no taken-action probability within a factor 2 of the 1e-8 clamp).  A row that misses one is redrawn when the
    case is built, so no row is ever left out of a comparison;
  * torch_qr / torch_c51 / torch_iqn: the reference's expressions on torch tensors of a chosen dtype (float32: what the
    reference itself computes; float64 with autograd: the independent check of the oracle's hand-derived gradients);
  * head_errors: the two error figures every comparison uses;
  * measure_fp32_reference_error: worst float32-reference error over a kernel's grid, the source of the named bounds
    in tests/test_dist_heads_gpu.py.
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch

from . import dist_oracle as O

F32 = np.float32
GAP_MIN = 1e-3                       # smallest allowed (best - second best) next-action value, as a share of the value scale
CLAMP_FACTOR = 2.0                   # no taken-action probability inside [1e-8 / 2, 1e-8 * 2]

GRID_A = (1, 3, 18)
GRID_B = (1, 5, 257)
GRID_LD_PAD = (0, 5)
QR_N = (1, 2, 51, 63, 64, 65, 128, 200, 256)
QR_KAPPA = (0.6, 1.0)
C51_N = (2, 3, 41, 51, 64, 65, 101, 256)
C51_SUPPORT = ((-10.0, 10.0), (0.0, 200.0))
IQN_NP = (1, 8, 64, 65, 200)
IQN_NPP = (1, 11, 128)
IQN_KAPPA = (0.6, 1.0)
GAMMA = 0.97


def seed_of(*key):
    return int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:4], "little")


def gap_ok(o):
    return o["gap"] >= GAP_MIN * o["value_scale"]


def clamp_ok(o):
    return o["clamp_margin"] > np.log(CLAMP_FACTOR)


def qr_grid():
    return [(N, A, B, k) for N in QR_N for A in GRID_A for B in GRID_B for k in QR_KAPPA]


def c51_grid():
    return [(N, A, B, s) for N in C51_N for A in GRID_A for B in GRID_B for s in C51_SUPPORT]


def iqn_grid():
    return [(Np, Npp, B, k) for Np in IQN_NP for Npp in IQN_NPP for B in GRID_B for k in IQN_KAPPA]


def _redraw(rng, arr, bad_rows, scale):
    arr[bad_rows] = (scale * rng.standard_normal((int(bad_rows.sum()),) + arr.shape[1:])).astype(F32)


def qr_case(N, A, B, seed=0):
    """Random (B, A, N) quantile tables, actions, rewards, dones for the QR head."""
    rng = np.random.default_rng(seed_of("qr", N, A, B, seed))
    c = dict(z_cur=rng.standard_normal((B, A, N)).astype(F32), z_next_online=rng.standard_normal((B, A, N)).astype(F32),
             z_next_target=(1.5 * rng.standard_normal((B, A, N))).astype(F32), actions=rng.integers(0, A, B).astype(np.int64),
             rew=rng.standard_normal(B).astype(F32), done=(rng.random(B) < 0.3).astype(F32))
    for _ in range(64):
        q = c["z_next_online"].astype(np.float64).mean(axis=2)
        _, gap, _ = O._first_argmax_and_gap(q)
        bad = gap < 2 * GAP_MIN * np.abs(c["z_next_online"]).max(axis=(1, 2))
        if not bad.any():
            return c
        _redraw(rng, c["z_next_online"], bad, 1.0)
    raise AssertionError("qr_case: could not separate the next-action values")


def c51_case(N, A, B, support, seed=0, cur_span=None):
    """Random (B, A, N) logits for the C51 head; rewards reach beyond both ends of the support.  cur_span: the online
    logits come in two bands `cur_span` nats apart (top band 8 nats wide, bottom band 8 nats wide), so the lower band's
    probabilities fall well below the 1e-8 clamp and the upper band's stay well above it."""
    v_min, v_max = support
    rng = np.random.default_rng(seed_of("c51", N, A, B, support, seed, cur_span))
    if cur_span is None:
        cur = 1.5 * rng.standard_normal((B, A, N))
    else:
        low = rng.random((B, A, N)) < 0.4
        cur = np.where(low, -cur_span + 8.0 * rng.random((B, A, N)), -8.0 * rng.random((B, A, N)))
        cur[:, :, 0] = 0.0                                    # one atom on top, one at the bottom: the full span in every row
        cur[:, :, -1] = -cur_span
    c = dict(logits_cur=cur.astype(F32), logits_next_target=(1.5 * rng.standard_normal((B, A, N))).astype(F32),
             actions=rng.integers(0, A, B).astype(np.int64),
             rew=(0.5 * (v_min + v_max) + 0.25 * (v_max - v_min) * rng.standard_normal(B)).astype(F32),
             done=(rng.random(B) < 0.3).astype(F32), support=torch.linspace(v_min, v_max, N).numpy(), v_min=v_min, v_max=v_max)
    sup = c["support"].astype(np.float64)
    for _ in range(64):
        p = np.exp(O._log_softmax(c["logits_next_target"].astype(np.float64)))
        _, gap, _ = O._first_argmax_and_gap((p * sup).sum(axis=2))
        bad = gap < 2 * GAP_MIN * np.abs(sup).max()
        if not bad.any():
            return c
        _redraw(rng, c["logits_next_target"], bad, 1.5)
    raise AssertionError("c51_case: could not separate the next-action values")


def iqn_case(Np, Npp, B, seed=0):
    rng = np.random.default_rng(seed_of("iqn", Np, Npp, B, seed))
    return dict(cur=rng.standard_normal((B, Np)).astype(F32), target=(1.5 * rng.standard_normal((B, Npp))).astype(F32),
                taus=rng.random((B, Np)).astype(F32))


# -- the reference's expressions on torch tensors of one dtype ---------------------------------------------------------
def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype)


def torch_qr(c, gamma, kappa, dtype):
    """qr_dqn_trainer.py:113-213 on the network outputs.  Returns (row terms of the loss, dloss/dz_cur, next actions)."""
    zc, zo, zt = (_t(c[k], dtype) for k in ("z_cur", "z_next_online", "z_next_target"))
    zc.requires_grad_(True)
    rew, done, act = _t(c["rew"], dtype), _t(c["done"], dtype), torch.as_tensor(c["actions"]).long()
    N = zc.shape[2]
    cur = zc.gather(1, act[:, None, None].expand(-1, -1, N)).squeeze(1)
    with torch.no_grad():
        nxt = torch.argmax(zo.mean(dim=2), dim=1, keepdim=True)
        nxt_q = zt.gather(1, nxt.unsqueeze(-1).expand(-1, -1, N)).squeeze(1)
        tgt = rew[:, None] + gamma * nxt_q * (1 - done[:, None])
    td = tgt.unsqueeze(2) - cur.unsqueeze(1)
    inside = (torch.abs(td) <= kappa).to(dtype)
    huber = inside * (0.5 * td.pow(2)) + (1 - inside) * (kappa * (torch.abs(td) - 0.5 * kappa))
    i = torch.arange(0, N, dtype=dtype)
    tau = ((2 * i + 1) / (2 * N)).unsqueeze(0)
    rho = torch.abs(tau.unsqueeze(-1) - (td < 0).to(dtype)) * huber
    rows = rho.sum(dim=2).mean(dim=1)
    rows.mean().backward()
    return rows.detach().numpy(), zc.grad.numpy(), nxt.squeeze(1).numpy()


def torch_c51(c, gamma, dtype):
    """c51_trainer.py:60-169 on the pre-softmax outputs (the reference's network ends in log_softmax over the atoms)."""
    lc, lt = _t(c["logits_cur"], dtype), _t(c["logits_next_target"], dtype)
    lc.requires_grad_(True)
    rew, done, act = _t(c["rew"], dtype), _t(c["done"], dtype), torch.as_tensor(c["actions"]).long()
    sup, v_min, v_max = _t(c["support"], dtype), float(c["v_min"]), float(c["v_max"])
    B, _, N = lc.shape
    delta = (v_max - v_min) / (N - 1)
    with torch.no_grad():
        p_next = torch.log_softmax(lt, dim=2).exp()
        nxt = torch.sum(p_next * sup[None, None, :], dim=2).argmax(1)
        p = p_next[range(B), nxt]
        tz = (rew.unsqueeze(1) + gamma * sup.unsqueeze(0) * (1 - done.unsqueeze(1))).clamp(v_min, v_max)
        b = (tz - v_min) / delta
        lo, up = b.floor().long(), b.ceil().long()
        m = torch.zeros_like(p)
        ne = lo != up
        m.scatter_add_(1, lo.clamp(0, N - 1), p * (up.to(dtype) - b) * ne)
        m.scatter_add_(1, up.clamp(0, N - 1), p * (b - lo.to(dtype)) * ne)
        m.scatter_add_(1, lo.clamp(0, N - 1), p * ~ne)
    logp = torch.log_softmax(lc, dim=2)[range(B), act]
    rows = -(m * logp.exp().clamp(min=1e-8).log()).sum(1)
    rows.mean().backward()
    return rows.detach().numpy(), lc.grad.numpy(), nxt.numpy(), m.numpy()


def torch_iqn(c, kappa, dtype):
    """iqn_trainer.py:128 and :137-149."""
    cur, tgt, taus = _t(c["cur"], dtype), _t(c["target"], dtype), _t(c["taus"], dtype)
    cur.requires_grad_(True)
    td = tgt.unsqueeze(1) - cur.unsqueeze(2)
    a = torch.abs(td)
    huber = torch.where(a <= kappa, 0.5 * td.pow(2), kappa * (a - 0.5 * kappa))
    rows = (torch.abs(taus.unsqueeze(-1) - (td < 0).to(dtype)) * huber).mean(dim=2).mean(dim=1)
    rows.mean().backward()
    return rows.detach().numpy(), cur.grad.numpy(), None


# -- error figures ------------------------------------------------------------------------------------------------------
def head_errors(row_loss, grad, o):
    """(loss error, gradient error) of one evaluation against the oracle result `o`, each the worst row's figure.
    gradient: largest |difference| in the row over the row's largest oracle gradient entry.  loss: |difference| over
    (|row loss| + B * largest gradient entry): a row whose loss is small only because u = T - theta cancels (N = 1, 2)
    is measured on the scale of u, which is where its rounding error lives, not on the scale of u^2."""
    B = len(o["row_loss"])
    g64 = o["grad"].reshape(B, -1)
    g = np.asarray(grad, dtype=np.float64).reshape(B, -1)
    gmax = np.abs(g64).max(axis=1)
    tiny = np.finfo(np.float64).tiny
    grad_err = (np.abs(g - g64).max(axis=1) / np.maximum(gmax, tiny)).max()
    loss_err = (np.abs(np.asarray(row_loss, dtype=np.float64) - o["row_loss"]) / np.maximum(np.abs(o["row_loss"]) + B * gmax, tiny)).max()
    return float(loss_err), float(grad_err)


def oracle_of(kernel, shape, c=None):
    """(case, oracle result) of one grid entry."""
    if kernel == "qr":
        N, A, B, kappa = shape
        c = c or qr_case(N, A, B)
        return c, O.qr_head(c["z_cur"], c["z_next_online"], c["z_next_target"], c["actions"], c["rew"], c["done"], GAMMA, kappa)
    if kernel == "c51":
        N, A, B, support = shape
        c = c or c51_case(N, A, B, support)
        return c, O.c51_head(c["logits_cur"], c["logits_next_target"], c["actions"], c["rew"], c["done"], c["support"], GAMMA,
                             c["v_min"], c["v_max"])
    Np, Npp, B, kappa = shape
    c = c or iqn_case(Np, Npp, B)
    return c, O.iqn_head(c["cur"], c["target"], c["taus"], kappa)


def fp32_reference(kernel, shape, c):
    if kernel == "qr":
        return torch_qr(c, GAMMA, shape[3], torch.float32)[:3]
    if kernel == "c51":
        return torch_c51(c, GAMMA, torch.float32)[:3]
    return torch_iqn(c, shape[3], torch.float32)


GRIDS = {"qr": qr_grid, "c51": c51_grid, "iqn": iqn_grid}


def measure_fp32_reference_error(kernel, shapes=None):
    """Worst (loss error, its shape, gradient error, its shape) of the float32 reference evaluation against the float64
    oracle over the kernel's grid (or over `shapes`)."""
    worst = [0.0, None, 0.0, None]
    for shape in (shapes or GRIDS[kernel]()):
        c, o = oracle_of(kernel, shape)
        rows, grad, nxt = fp32_reference(kernel, shape, c)
        if nxt is not None:
            assert gap_ok(o).all() and np.array_equal(nxt, o["next_action"]), shape
        le, ge = head_errors(rows, grad, o)
        if le > worst[0]:
            worst[0], worst[1] = le, shape
        if ge > worst[2]:
            worst[2], worst[3] = ge, shape
    return tuple(worst)


# -- trainer-level cases ------------------------------------------------------------------------------------------------
def mlp_case(S, n_out, hidden, B, A, seed, reward_scale=1.0, out_scale=1.0):
    """Online and target parameters ((W, b) per Linear, nn.Linear's uniform(+-1/sqrt(fan_in)) ranges, the output layer
    times out_scale; the target is the online net plus 0.05-sigma noise) and one minibatch."""
    rng = np.random.default_rng(seed_of("mlp", S, n_out, tuple(hidden), B, A, seed))
    dims = [S] + list(hidden) + [n_out]
    online = []
    for d_in, d_out in zip(dims[:-1], dims[1:]):
        k = 1.0 / np.sqrt(d_in)
        online.append((rng.uniform(-k, k, (d_out, d_in)).astype(F32), rng.uniform(-k, k, d_out).astype(F32)))
    online[-1] = tuple((out_scale * v).astype(F32) for v in online[-1])
    target = [((W + 0.05 * rng.standard_normal(W.shape)).astype(F32), (b + 0.05 * rng.standard_normal(b.shape)).astype(F32))
              for W, b in online]
    return dict(online=online, target=target, states=(3.0 * rng.standard_normal((B, S))).astype(F32),
                next_states=(3.0 * rng.standard_normal((B, S))).astype(F32), actions=rng.integers(0, A, B).astype(np.int64),
                rew=(reward_scale * rng.standard_normal(B)).astype(F32), done=(rng.random(B) < 0.2).astype(F32))


def mlp_forward64(layers, x):
    """Linear/ReLU stack in float64."""
    h = np.asarray(x, dtype=np.float64)
    for i, (W, b) in enumerate(layers):
        h = h @ W.astype(np.float64).T + b.astype(np.float64)
        if i < len(layers) - 1:
            h = np.maximum(h, 0.0)
    return h


# one learn() of the trainers at their class defaults ([128, 128], 51 quantiles / atoms, C51 on [-10, 10]), and QR-DQN with
# the QR-DQN paper's 200 quantiles on 5 actions (a 1000-wide output layer).  The seeds are the first ones whose rows all
# meet the gap condition (tests/test_dist_oracle.py checks that they do).
TRAINER_CASES = {
    "qr_default": dict(kind="qr", S=8, A=4, N=51, hidden=(128, 128), B=64, gamma=0.99, kappa=1.0, seed=4),
    "qr_n200_a5": dict(kind="qr", S=8, A=5, N=200, hidden=(128, 128), B=64, gamma=0.99, kappa=1.0, seed=32),
    "c51_default": dict(kind="c51", S=8, A=4, N=51, hidden=(128, 128), B=64, gamma=0.99, v_min=-10.0, v_max=10.0, seed=4,
                        reward_scale=6.0, out_scale=4.0),
}
# greedy-action epilogue of the act kernel: kind 2 (QR mean) and kind 1 (C51 expectation) at 51 and at A * n_sub = 1000
ACT_CASES = {
    "qr_n51": dict(kind="qr", S=8, A=4, N=51, hidden=(128, 128), B=12, seed=0),
    "qr_1000": dict(kind="qr", S=8, A=5, N=200, hidden=(128, 128), B=12, seed=2),
    "c51_n51": dict(kind="c51", S=8, A=4, N=51, hidden=(128, 128), B=12, v_min=-10.0, v_max=10.0, seed=0, out_scale=4.0),
    "c51_1000": dict(kind="c51", S=8, A=5, N=200, hidden=(128, 128), B=12, v_min=-10.0, v_max=10.0, seed=0, out_scale=4.0),
}


def trainer_case(spec):
    """(minibatch and parameters, float64 oracle of the loss head on float64 forward passes, oracle dL/d(output bias))."""
    A, N, B = spec["A"], spec["N"], spec["B"]
    c = mlp_case(spec["S"], A * N, spec["hidden"], B, A, spec["seed"], spec.get("reward_scale", 1.0), spec.get("out_scale", 1.0))
    fwd = lambda layers, x: mlp_forward64(layers, x).reshape(B, A, N)
    if spec["kind"] == "qr":
        o = O.qr_head(fwd(c["online"], c["states"]), fwd(c["online"], c["next_states"]), fwd(c["target"], c["next_states"]),
                      c["actions"], c["rew"], c["done"], spec["gamma"], spec["kappa"])
    else:
        c["support"] = torch.linspace(spec["v_min"], spec["v_max"], N).numpy()
        o = O.c51_head(fwd(c["online"], c["states"]), fwd(c["target"], c["next_states"]), c["actions"], c["rew"], c["done"],
                       c["support"], spec["gamma"], spec["v_min"], spec["v_max"])
    return c, o, o["grad"].reshape(B, A * N).sum(axis=0)


def act_case(spec):
    """(parameters and states, oracle greedy action per state, gap, value scale) of the act epilogue."""
    A, N, B = spec["A"], spec["N"], spec["B"]
    c = mlp_case(spec["S"], A * N, spec["hidden"], B, A, ("act", spec["seed"]), out_scale=spec.get("out_scale", 1.0))
    out = mlp_forward64(c["online"], c["states"]).reshape(B, A, N)
    if spec["kind"] == "qr":
        best, gap, _ = O._first_argmax_and_gap(out.mean(axis=2))
        scale = np.abs(out).max(axis=(1, 2))
    else:
        c["support"] = torch.linspace(spec["v_min"], spec["v_max"], N).numpy()
        sup = c["support"].astype(np.float64)
        best, gap, _ = O._first_argmax_and_gap((np.exp(O._log_softmax(out)) * sup).sum(axis=2))
        scale = np.full(B, np.abs(sup).max())
    return c, best, gap, scale


# -- edge cases -----------------------------------------------------------------------------------------------------------
def qr_edge_cases():
    """name -> (case, gamma, kappa, exact): the boundary cases of the QR head.  exact: every quantity of the case is a
    small dyadic rational, so float32 and float64 take the same branches and produce the same numbers, bit for bit."""
    out = {}
    c = qr_case(65, 3, 5, seed="done")
    c["done"][:] = 1.0
    out["done_all"] = (c, GAMMA, 0.6, False)
    out["gamma_zero"] = (qr_case(65, 3, 5, seed="gamma0"), 0.0, 1.0, False)
    # integers in [-2, 2], gamma = kappa = 1, tau_i = (2i + 1) / (2N) with N a power of two, B = 8: u is an integer, |u| == kappa
    # and u == 0 both occur, and every sum is exact in float32 (terms are multiples of 2^-8 and the totals stay below 2^14)
    for N in (4, 64):
        rng = np.random.default_rng(seed_of("qr-int", N))
        B, A = 8, 2
        ints = lambda *shape: rng.integers(-2, 3, shape).astype(F32)
        c = dict(z_cur=ints(B, A, N), z_next_online=ints(B, A, N), z_next_target=ints(B, A, N),
                 actions=rng.integers(0, A, B).astype(np.int64), rew=ints(B), done=(rng.random(B) < 0.3).astype(F32))
        c["z_next_online"][:, 0, :] += (10.0 * rng.integers(0, 2, B).astype(F32) - 5.0)[:, None]   # means >= 1 apart: no accidental tie
        out[f"integers_n{N}"] = (c, 1.0, 1.0, True)
    # exact tie of two action means at N = 200: the tied rows hold 0.5 everywhere and 0.25 / 0.75 alternating (both sum to 100
    # exactly in any order), the others lie lower; torch.argmax takes the first of the two
    B, A, N = 6, 4, 200
    c = qr_case(N, A, B, seed="tie")
    pairs = [(0, 2), (1, 3), (1, 2), (0, 3), (2, 3), (0, 1)]
    flat, wavy = np.full(N, 0.5, F32), np.where(np.arange(N) % 2 == 0, 0.25, 0.75).astype(F32)
    for b, (first, second) in enumerate(pairs):
        c["z_next_online"][b] = np.where(np.arange(N) % 4 == 0, -1.0, 0.5).astype(F32)   # mean 0.125
        c["z_next_online"][b, first] = wavy if b % 2 else flat
        c["z_next_online"][b, second] = flat if b % 2 else wavy
    c["tie_first"] = np.array([p[0] for p in pairs])
    out["tie_n200"] = (c, GAMMA, 1.0, False)
    return out


def c51_edge_cases():
    """name -> case of the C51 head's boundary cases (all on 41 atoms over [-10, 10] unless the name says otherwise; with
    delta_z = 0.5 every atom is exact in float32).  `uniform_cur`: the online logits are zero, so p = 1/N, the clamp mask is
    one everywhere and the projected distribution can be read back from the gradient, m_k = 1/N - B * dl_k."""
    out = {}
    sup = (-10.0, 10.0)
    c = c51_case(65, 3, 5, sup, seed="far")
    c["rew"][:] = np.where(np.arange(5) % 2 == 0, 1000.0, -1000.0)
    out["rewards_far_beyond"] = dict(c, gamma=GAMMA)
    c = c51_case(65, 3, 5, sup, seed="done")
    c["done"][:] = 1.0
    out["done_all"] = dict(c, gamma=GAMMA)
    for N, s in ((51, sup), (65, sup), (256, (0.0, 200.0))):
        c = c51_case(N, 3, 37, s, seed="uniform")
        c["logits_cur"][:] = 0.0
        out[f"uniform_cur_n{N}"] = dict(c, gamma=GAMMA, uniform_cur=True)
    c = c51_case(41, 3, 9, sup, seed="identity")
    c["logits_cur"][:] = 0.0
    c["rew"][:], c["done"][:] = 0.0, 0.0
    out["exact_hits_identity"] = dict(c, gamma=1.0, uniform_cur=True, identity=True)
    c = c51_case(41, 3, 9, sup, seed="onehot")
    c["logits_cur"][:] = 0.0
    c["done"][:] = 1.0
    c["rew"][:] = np.array([-10.0, -9.5, -3.0, 0.0, 0.5, 4.5, 9.5, 10.0, 12.5], F32)     # multiples of delta_z; the last clamps
    out["exact_hits_one_atom"] = dict(c, gamma=GAMMA, uniform_cur=True, one_atom=True)
    for N in (51, 200):
        out[f"clamp_branch_n{N}"] = dict(c51_case(N, 3, 37, sup, seed="clamp", cur_span=30.0), gamma=GAMMA, clamped=True)
    return out


def c51_oracle(c, gamma):
    return O.c51_head(c["logits_cur"], c["logits_next_target"], c["actions"], c["rew"], c["done"], c["support"], gamma,
                      c["v_min"], c["v_max"])


def qr_oracle(c, gamma, kappa):
    return O.qr_head(c["z_cur"], c["z_next_online"], c["z_next_target"], c["actions"], c["rew"], c["done"], gamma, kappa)
