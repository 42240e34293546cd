"""Seeded cases of the Q-network learn step (csrc/qnet_fused.hpp's three step kernels and the multi-launch path of
csrc/qnet_api.inc with cql_loss_kernel), shared by the CPU checks (tests/test_qstep_cases.py) and the GPU comparison
(tests/test_qstep_gpu.py): parameters, replay arrays, the variant's extra inputs, Adam moments, a minibatch drawn from
rows on which the step is continuous, and the step itself in fp64 (`step64`, the yardstick) and in fp32 (`step32`, the
control that sets the GPU bars).  numpy only.

The step, from include/porl_hip.h (porl_qnet_variant) and the header of cql_loss_kernel (csrc/kernels.hpp):
    y      = r + gamma * Q_target(s')[a*] * (1 - d)
    a*     = argmax Q_target(s')                          plain
             first argmax of Q_online(s')                 Double DQN
             first maximum of Q_target(s') over the allowed actions, action 0 when none is allowed      BCQ mask
    diff   = Q(s)[a] - y                                  (0 with td_off)
    wgt    = is_w[b] * w_uniform                          (absent factors are 1)
    td     = 1/B sum_b wgt * diff^2,   pen = 1/B sum_b (logsumexp Q(s) - ln A - Q(s)[a]),   loss = td + alpha * pen
    dL/dQ  = alpha/B * softmax + 1[j = a] * (2/B * wgt * diff - alpha/B)
(The kernels form the masked pick as argmax [q + (mask - 1) * 1e10] in fp32, where the sum absorbs q: every disallowed
entry is exactly -1e10, and a row without an allowed action ties at index 0.  In fp64 the sum does not absorb q, so the
oracle states the rule instead of evaluating the expression.)

Its only discontinuities are the ReLUs of the online network on s (they gate gradients) and the Double-DQN argmax of
Q_online(s').  A replay row is DECIDED when, in fp64, every hidden pre-activation of the online network on s has
|z| >= MARGIN and the two largest entries of Q_online(s') are MARGIN apart (or tie exactly by construction: the tie
case).  `idx` is drawn from decided rows only, so no comparison has to leave a row out."""
import itertools
import zlib

import numpy as np

MARGIN = 1e-4
GAMMA = 0.97
LR, STEP, BETAS, EPS = 5e-4, 3, (0.9, 0.999), 1e-8
W_UNIFORM = 0.37

# name: (S, hidden, B, why)
SHAPES = {
    "row1": (5, (7,), 1, "a single-row batch"),
    "odd": (17, (32, 96), 33, "2x16+1 and 32+1 rows: a one-row last block in both block sizes"),
    "deep": (12, (40, 33, 128, 20), 31, "five Linear layers, the kernels' limit; a 24-tile layer: wgrad_share active"),
    "maxk": (128, (128, 128), 17, "widest input and layers: one weight image fills LDS, the one-group kernel in every "
                                    "one-launch form"),
    "blocks": (5, (7,), 1025, "65 sixteen-row blocks: the reduce kernel's second trip"),
}
ACTIONS = (2, 4, 5, 8, 9, 13, 16, 17, 24, 25, 32, 33, 64, 128)
# name: alpha, double_dqn, next_mask, is_w, w_uniform, td_abs requested, td_off
VARIANTS = {
    "cql": dict(alpha=0.7),
    "dqn": dict(alpha=0.0),
    "double_dqn": dict(alpha=0.7, double_dqn=True, td_abs=True),
    "bcq_mask": dict(alpha=0.7, mask=True, td_abs=True),
    "per": dict(alpha=0.0, double_dqn=True, is_w=True, td_abs=True),
    "per_uniform": dict(alpha=0.0, double_dqn=True, w_uniform=True, td_abs=True),
    "both_weights": dict(alpha=0.7, is_w=True, w_uniform=True),
    "td_off": dict(alpha=1.0, td_off=True, td_abs=True),
}
TIE_PAIR = (1, 3)            # output units j1 < j2 of the online net made identical in the tie case


def variant(case):
    v = dict(alpha=0.0, double_dqn=False, mask=False, is_w=False, w_uniform=False, td_abs=False, td_off=False)
    v.update(VARIANTS[case["variant"]])
    return v


def loss_path(A, masked):
    """Which loss stage of qnet_fused.hpp a case takes: rows8, regs<NC> or the run-time loop."""
    if A > 32:
        return "loop"
    if not masked:
        return "rows8"
    nc = (A + 3) >> 2
    return f"regs{nc if nc <= 4 else (6 if nc <= 6 else 8)}"


def case(shape, A, var, tie=False):
    """A named case; CASES below is the grid, tests may form further ones."""
    S, hidden, B, why = SHAPES[shape]
    path = loss_path(A, VARIANTS[var].get("mask", False))
    covers = f"{why}; A={A}: loss stage {path}, {(A + 31) // 32} output tile(s); {var}"
    if tie:
        covers += f"; online outputs {TIE_PAIR[0]} and {TIE_PAIR[1]} identical: exact argmax ties"
    return dict(name=f"{shape}-a{A}-{var}" + ("-tie" if tie else ""), shape=shape, S=S, hidden=hidden, B=B, A=A, variant=var,
                tie=tie, covers=covers)


# The full A x variant product on `odd`; A in {5, 33} x every variant on the other shapes (`blocks` included: 16 steps of
# 1025 rows on a 5-7-A network cost less than the 112 of `odd`); one designed tie case.
CASES = [case("odd", A, v) for A, v in itertools.product(ACTIONS, VARIANTS)]
CASES += [case(s, A, v) for s in ("row1", "deep", "maxk", "blocks") for A, v in itertools.product((5, 33), VARIANTS)]
CASES += [case("odd", 5, "double_dqn", tie=True)]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def n_lin(case):
    return len(case["hidden"]) + 1


def _forward(params, x, dtype):
    """-> (Q, [input of layer l], [pre-activation of hidden layer l])."""
    h = x.astype(dtype)
    ins, zs = [], []
    n = len(params) // 2
    for l in range(n):
        ins.append(h)
        z = h @ params[2 * l].astype(dtype).T + params[2 * l + 1].astype(dtype)
        if l < n - 1:
            zs.append(z)
            h = np.maximum(z, dtype(0))
        else:
            h = z
    return h, ins, zs


def _top2_gap(q):
    if q.shape[1] < 2:
        return np.full(q.shape[0], np.inf)
    s = np.sort(q, axis=1)
    return s[:, -1] - s[:, -2]


def _decided_rows(case, online, states, next_states):
    """(decided, tie) boolean arrays over all replay rows, in fp64."""
    _, _, zs = _forward(online, states, np.float64)
    ok = np.ones(states.shape[0], dtype=bool)
    for z in zs:
        ok &= (np.abs(z) >= MARGIN).all(axis=1)
    qn, _, _ = _forward(online, next_states, np.float64)
    gap = _top2_gap(qn)
    tie = np.zeros_like(ok)
    if case["tie"]:
        j1, j2 = TIE_PAIR
        rest = np.delete(qn, [j1, j2], axis=1).max(axis=1)
        tie = (qn[:, j1] == qn[:, j2]) & (qn[:, j1] - rest >= MARGIN)
    return ok & ((gap >= MARGIN) | tie), tie


def make(case):
    S, hidden, B, A = case["S"], case["hidden"], case["B"], case["A"]
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    dims = [S] + list(hidden) + [A]
    nets = []
    for _ in range(2):                                   # online, target
        p = []
        for l in range(len(dims) - 1):
            p.append((1.4 * rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32))
            p.append((0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32))
        nets.append(p)
    online, target = nets
    N = 3 * B + 7
    states = rng.standard_normal((N, S)).astype(np.float32)
    next_states = rng.standard_normal((N, S)).astype(np.float32)
    if case["tie"]:
        # both units of the pair take the weights of the unit that wins most often on s', so the pair is often the maximum
        k = np.bincount(_forward(online, next_states, np.float64)[0].argmax(axis=1), minlength=A).argmax()
        w, b = online[-2][k].copy(), online[-1][k].copy()
        for j in TIE_PAIR:
            online[-2][j], online[-1][j] = w, b
    actions = rng.integers(0, A, N).astype(np.int64)
    rewards = rng.standard_normal(N).astype(np.float32)
    dones = (rng.uniform(size=N) < 0.25).astype(np.float32)
    mask = (rng.uniform(size=(B, A)) < 0.6).astype(np.float32)
    if B >= 3:
        mask[1], mask[2] = 0.0, 1.0
    is_w = rng.uniform(0.2, 1.0, B).astype(np.float32)
    # Moments of a run in progress.  |m| stays below ~2e-3: where m + (1 - beta1) (g - m) cancels, fp32 leaves an absolute
    # error of about half an ulp of each term (ulp(2e-3) = 2.3e-10), which the fp64 comparison of the Adam fold has to
    # take at its 1e-9 absolute bar; sqrt(v) >= 5e-3 keeps m / sqrt(v) of order one.
    adam_m = [(5e-4 * rng.standard_normal(p.shape)).astype(np.float32) for p in online]
    adam_v = [((0.01 * (0.5 + np.abs(rng.standard_normal(p.shape)))) ** 2).astype(np.float32) for p in online]
    decided, tie = _decided_rows(case, online, states, next_states)
    pool = np.flatnonzero(decided)
    if len(pool) < B:
        raise ValueError(f"{case['name']}: {len(pool)} decided rows for a batch of {B}")
    masked = VARIANTS[case["variant"]].get("mask", False)
    qt_argmax = _forward(target, next_states, np.float64)[0].argmax(axis=1)
    idx = None
    for _ in range(200):          # seeded redraws until the batch shows what the case is there to show
        idx = rng.permutation(pool)[:B].astype(np.int64)
        if B > 1 and (np.diff(idx) > 0).all():
            continue
        if B >= 17 and len(np.unique(dones[idx])) < 2:
            continue
        if case["tie"] and int((tie[idx] & (dones[idx] == 0)).sum()) < 3:
            continue
        if masked and B >= 3 and (dones[idx[1]] != 0 or qt_argmax[idx[1]] == 0):
            continue              # the all-zero mask row must show its pick: not terminal, action 0 not the plain maximum
        break
    else:
        raise ValueError(f"{case['name']}: no admissible minibatch")
    return dict(case=case, online=online, target=target, states=states, next_states=next_states, actions=actions,
                rewards=rewards, dones=dones, mask=mask, is_w=is_w, w_uniform=np.float32(W_UNIFORM), adam_m=adam_m,
                adam_v=adam_v, idx=idx, n_rows=N, n_decided=int(decided.sum()), tie_rows=tie[idx])


def bootstrap_action(v, q_target_next, q_online_next, mask):
    """The action whose target-network value enters y, per row."""
    if v["double_dqn"]:
        return np.argmax(q_online_next, axis=1)
    if v["mask"]:
        allowed = mask > 0.5
        masked = np.where(allowed, q_target_next, -np.inf)
        return np.where(allowed.any(axis=1), np.argmax(masked, axis=1), 0)
    return np.argmax(q_target_next, axis=1)


def _step(d, dtype):
    case = d["case"]
    v = variant(case)
    B, A = case["B"], case["A"]
    f = dtype
    idx = d["idx"]
    xs, xn = d["states"][idx], d["next_states"][idx]
    act = d["actions"][idx]
    rew, done = d["rewards"][idx].astype(f), d["dones"][idx].astype(f)
    ar = np.arange(B)
    q, ins, zs = _forward(d["online"], xs, f)
    qt, _, _ = _forward(d["target"], xn, f)
    qo = _forward(d["online"], xn, f)[0] if v["double_dqn"] else None
    boot = bootstrap_action(v, qt, qo, d["mask"])
    y = rew + f(GAMMA) * qt[ar, boot] * (f(1) - done)
    qa = q[ar, act]
    diff = np.zeros(B, dtype=f) if v["td_off"] else qa - y
    wgt = np.ones(B, dtype=f)
    if v["is_w"]:
        wgt = wgt * d["is_w"].astype(f)
    if v["w_uniform"]:
        wgt = wgt * f(d["w_uniform"])
    inv_b = f(1) / f(B)
    alpha = f(v["alpha"])
    mx = q.max(axis=1, keepdims=True)
    e = np.exp(q - mx)
    se = e.sum(axis=1, keepdims=True)
    lse = (mx + np.log(se))[:, 0]
    td = (wgt * diff * diff).sum() * inv_b
    pen = (lse - f(np.log(f(A))) - qa).sum() * inv_b
    dq = alpha * inv_b * (e / se)
    dq[ar, act] += f(2) * inv_b * wgt * diff - alpha * inv_b
    grads = [None] * len(d["online"])
    dz = dq
    for l in range(len(ins) - 1, -1, -1):
        grads[2 * l] = dz.T @ ins[l]
        grads[2 * l + 1] = dz.sum(axis=0)
        if l > 0:
            dz = (dz @ d["online"][2 * l].astype(f)) * (zs[l - 1] > 0)
    return dict(td_abs=np.abs(diff), stats=np.array([td + alpha * pen, td, pen], dtype=f), grads=grads, boot=boot,
                q_target_next=qt, y_terms=(rew, done, qa))


def step64(d):
    return _step(d, np.float64)


def step32(d):
    return _step(d, np.float32)


def td_abs_for_action(d, ref, j):
    """fp64 |Q(s)[a] - y| per row if every row bootstrapped from action j: what td_abs would show for that pick."""
    rew, done, qa = ref["y_terms"]
    return np.abs(qa - (rew + GAMMA * ref["q_target_next"][:, j] * (1.0 - done)))


def errors(ref64, got):
    """Error of `got` (the fp32 control, or a kernel) against the fp64 step, per quantity: td_abs and stats as the largest
    absolute error over max(1, max-abs of the fp64 values), each gradient tensor as its largest absolute error over its own
    fp64 max-abs."""
    rel = lambda x, r: float(np.abs(np.asarray(x, dtype=np.float64) - r).max() / max(1.0, float(np.abs(r).max())))
    return dict(td_abs=rel(got["td_abs"], ref64["td_abs"]), stats=rel(got["stats"], ref64["stats"]),
                grads=[float(np.abs(np.asarray(g, dtype=np.float64) - g64).max() / grad_scale(g64))
                       for g, g64 in zip(got["grads"], ref64["grads"])])


def grad_scale(g64):
    s = float(np.abs(g64).max())
    return s if s > 0.0 else 1.0


def adam64(p, g, m, v, lr=LR, step=STEP, betas=BETAS, eps=EPS):
    """torch.optim.Adam's update (no weight decay, no amsgrad) in fp64 -> (p, m, v)."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    b1, b2 = betas
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * m / denom, m, v
