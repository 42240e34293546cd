"""float64 oracle of the three distributional loss heads (csrc/dist_losses.hpp).

TEST INFRASTRUCTURE ONLY.  Plain numpy restatements, in broadcast form, of the reference's expressions:

  qr_head   QRDQNTrainer.learn        (src/porl/train/qr_dqn_trainer.py:109-213)
  c51_head  C51Trainer.learn          (src/porl/train/c51_trainer.py:52-169)
  iqn_head  IQNTrainer.quantile_huber_loss on td = target.unsqueeze(1) - current.unsqueeze(2)   (iqn_trainer.py:128,137-149)

Each returns a dict with the per-row loss terms (`row_loss`, whose batch mean is the reference's scalar loss), the
analytic gradient of that batch-mean loss with respect to the online network's output on `s` (`grad`), the chosen next
action (`next_action`; None for the IQN head, which receives its target already gathered) and the diagnostics the tests
use as input conditions: `gap`, the per-row distance between the best and the second-best next-action value (inf with
one action), `value_scale`, the scale on which such a value rounds (QR: the row's largest |quantile| of the online net on
s'; C51: the largest |atom| of the support), and for C51 `clamp_margin`, the smallest
|log(p_n / 1e-8)| over the taken action's atoms.  The gradients are hand-derived; tests/test_dist_oracle.py checks them
against torch.autograd in float64 and against the reference's own float32 numbers (tests/golden/*_head_*.npz).

Nothing here imports porl_amd, and nothing follows the kernels' loop structure.
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
CLAMP_MIN = 1e-8                  # c51_trainer.py:168, .clamp(min=1e-8)


def _f(x):
    return np.asarray(x, dtype=F64)


def _first_argmax_and_gap(q):
    """q (B, A) -> (first maximum per row, top-1 minus top-2 (inf when A == 1), largest |q| per row)."""
    best = np.argmax(q, axis=1)
    if q.shape[1] == 1:
        gap = np.full(q.shape[0], np.inf)
    else:
        top = np.sort(q, axis=1)
        gap = top[:, -1] - top[:, -2]
    return best, gap, np.abs(q).max(axis=1)


def _huber(u, kappa):
    """(L_kappa(u), dL_kappa/du): quadratic where |u| <= kappa, linear outside."""
    au = np.abs(u)
    quad = au <= kappa
    return np.where(quad, 0.5 * u * u, kappa * (au - 0.5 * kappa)), np.where(quad, u, kappa * np.sign(u))


def qr_head(z_cur, z_next_online, z_next_target, actions, rew, done, gamma, kappa):
    """z_* (B, A, N).  loss = mean_b mean_i sum_j |tau_i - 1[u_ij < 0]| L_kappa(u_ij), u_ij = T_i - theta_j: i runs over the
    TARGET quantiles and carries tau (`self.tau.unsqueeze(-1)` against a (B, N_target, N_current) error), j over the
    current ones."""
    zc, zo, zt = _f(z_cur), _f(z_next_online), _f(z_next_target)
    B, A, N = zc.shape
    actions = np.asarray(actions, dtype=np.int64)
    rows = np.arange(B)
    best, gap, _ = _first_argmax_and_gap(zo.mean(axis=2))
    scale = np.abs(zo).max(axis=(1, 2))                   # the values being averaged set the rounding scale of a mean
    T =_f(rew)[:, None] + gamma * zt[rows, best] * (1.0 - _f(done))[:, None]            # (B, N) over i
    theta = zc[rows, actions]                                                            # (B, N) over j
    u = T[:, :, None] - theta[:, None, :]                                                # (B, i, j)
    tau = (2.0 * np.arange(N) + 1.0) / (2.0 * N)
    w = np.abs(tau[None, :, None] - (u < 0))
    L, dL = _huber(u, kappa)
    grad = np.zeros_like(zc)
    grad[rows, actions] = -(w * dL).sum(axis=1) / (B * N)                                # du/dtheta_j = -1
    return dict(row_loss=(w * L).sum(axis=(1, 2)) / N, grad=grad, next_action=best, gap=gap, value_scale=scale, target=T)


def c51_project(p_next, rew, done, support, gamma, v_min, v_max):
    """Categorical projection (c51_trainer.py:90-149) of p_next (B, N) onto the support, as one (B, N, N) product."""
    N = p_next.shape[1]
    sup = _f(support)
    delta = (F64(v_max) - F64(v_min)) / (N - 1)
    tz = np.clip(_f(rew)[:, None] + gamma * sup[None, :] * (1.0 - _f(done))[:, None], v_min, v_max)
    b = (tz - v_min) / delta
    lo, up = np.floor(b), np.ceil(b)
    exact = lo == up
    w_lo = np.where(exact, 1.0, up - b)                   # an exact hit leaves all of its mass on atom l
    w_up = np.where(exact, 0.0, b - lo)
    k = np.arange(N)[None, None, :]
    lo_i = np.clip(lo, 0, N - 1).astype(np.int64)[:, :, None]
    up_i = np.clip(up, 0, N - 1).astype(np.int64)[:, :, None]
    share = w_lo[:, :, None] * (k == lo_i) + w_up[:, :, None] * (k == up_i)              # (B, source n, destination k)
    return (p_next[:, :, None] * share).sum(axis=1)


def _log_softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


def c51_head(logits_cur, logits_next_target, actions, rew, done, support, gamma, v_min, v_max):
    """logits_* (B, A, N), pre-softmax.  loss = -mean_b sum_n m_n log(clamp(p_n, 1e-8)) with p = softmax of the taken
    action's logits; clamp passes gradient where p_n >= 1e-8 (mask c), so with S = sum_n c_n m_n
    dL/dlogit_k = -(1/B) (c_k m_k - p_k S)."""
    lc, lt = _f(logits_cur), _f(logits_next_target)
    B, A, N = lc.shape
    actions = np.asarray(actions, dtype=np.int64)
    rows = np.arange(B)
    p_next = np.exp(_log_softmax(lt))
    best, gap, _ = _first_argmax_and_gap((p_next * _f(support)[None, None, :]).sum(axis=2))
    scale = np.full(B, np.abs(_f(support)).max())         # an expectation over the support rounds at the support's scale
    m =c51_project(p_next[rows, best], rew, done, support, gamma, v_min, v_max)
    logp = _log_softmax(lc[rows, actions])
    p = np.exp(logp)
    c = p >= CLAMP_MIN
    row_loss = -(m * np.log(np.maximum(p, CLAMP_MIN))).sum(axis=1)
    grad = np.zeros_like(lc)
    grad[rows, actions] = -(c * m - p * (c * m).sum(axis=1, keepdims=True)) / B
    return dict(row_loss=row_loss, grad=grad, next_action=best, gap=gap, value_scale=scale, m=m,
                clamp_margin=np.abs(logp - np.log(CLAMP_MIN)).min(axis=1))


def iqn_head(cur, target, taus, kappa):
    """cur, taus (B, N'), target (B, N'').  u_ij = target_j - cur_i; tau belongs to the CURRENT quantile i;
    loss = mean over (b, i, j)."""
    cur, target, taus = _f(cur), _f(target), _f(taus)
    B, Np = cur.shape
    Npp = target.shape[1]
    u = target[:, None, :] - cur[:, :, None]
    w = np.abs(taus[:, :, None] - (u < 0))
    L, dL = _huber(u, kappa)
    return dict(row_loss=(w * L).mean(axis=(1, 2)), grad=-(w * dL).sum(axis=2) / (B * Np * Npp), next_action=None)
