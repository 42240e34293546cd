"""Shared inputs of the IQN online tests (tests/test_iqn_online.py on the CPU, tests/test_iqn_online_gpu.py on the device):
the greedy-action cases — seeded network, 32 states, fixed fractions — with the fp64 oracle's answer and the states whose
top-two gap is wide enough for exact action equality to mean something; and, below them, the cases of the engine grid
(tests/test_iqn_cases.py, tests/test_iqn_engine_gpu.py)."""
import itertools
import zlib

import numpy as np
import torch

from oracle import iqn_oracle as IO

ACT_S, ACT_A, ACT_E, ACT_STATES = 11, 5, 16, 32
ACT_CASES = [(32, 1), (32, 32), (512, 1), (512, 32)]          # (hidden, N_policy)
ACT_SEED = 3
ACT_MIN_GAP = 1e-4


def act_case(H, n_policy):
    """-> (state_dict as numpy, states (32, S) float32, taus (32, n_policy) float32, oracle actions, keep mask)."""
    from porl_amd.net.iqn_network import IQNNetwork
    torch.manual_seed(ACT_SEED)
    net = IQNNetwork(ACT_S, ACT_A, ACT_E, H)                   # built on the CPU: the weights a seeded trainer gets
    P = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    P["value_net.2.bias"][:] = 0.0                             # a default-initialised head answers with its largest bias
    P["value_net.2.weight"] *= 4.0
    rng = np.random.default_rng(1000 * H + n_policy)
    states = (1.5 * rng.standard_normal((ACT_STATES, ACT_S))).astype(np.float32)
    taus = rng.random((ACT_STATES, n_policy)).astype(np.float32)
    P64 = {k: v.astype(np.float64) for k, v in P.items()}
    q = IO.forward(P64, states.astype(np.float64), taus.astype(np.float64)).mean(1)      # (32, A)
    top = np.sort(q, axis=1)
    keep = (top[:, -1] - top[:, -2]) >= ACT_MIN_GAP
    return P, states, taus, q.argmax(1), keep


# =====================================================================================================================
# Cases of the IQN ENGINE (csrc/iqn_api.inc, the second half of csrc/iqn.hpp), shared by tests/test_iqn_cases.py on the CPU
# and tests/test_iqn_engine_gpu.py on the device.  numpy only, every draw from a seed derived from the case's name.
#
# The learn step's only discontinuities are the ReLUs of the online network on (s, tau') — on h0, feat and v0 — and the
# Double-DQN argmax of the tau''-mean of the online network on s' (the quantile-Huber loss is C1).  A SAMPLE is a replay
# row together with its fractions; it is DECIDED when, in fp64, every such pre-activation has |z| >= MARGIN and the two
# largest means are MARGIN apart (or tie exactly by construction: the tie case).  Candidates are drawn from the seed and
# the decided ones kept until the minibatch is full, so no comparison has to leave a sample out.
# =====================================================================================================================
MARGIN = 1e-4                # tests/helpers/qstep_cases.py's
GAMMA = 0.97
LR, STEP, BETAS, EPS = 5e-4, 3, (0.9, 0.999), 1e-8
TIE_PAIR = (1, 3)             # rows j1 < j2 of value_net.2 made identical in the tie case
MAX_E, MAX_TAU, MAX_A = 128, 256, 64                  # IQN_MAX_E, IQN_MAX_TAU, IQN_MAX_A of csrc/iqn.hpp
MIX_ROWS, MIX_COLS, WG_T, WG_ROWS = 32, 64, 16, 128   # IQN_MIX_ROWS, IQN_MIX_COLS, IQN_WG_T, IQN_WG_ROWS

# name: (S, H, E, A, B, N', N'', what the shape is the smallest to reach)
LEARN_SHAPES = {
    "one": (1, 5, 1, 3, 1, 1, 1, "a single row; Hp = 8 > H = 5; a one-feature embedding"),
    "ragged": (13, 30, 10, 5, 37, 3, 5, "H % 4 = 2: three padding columns per workspace row and parameter rows off the "
                                        "16-byte grid; E % 8 != 0: the k < E tail of the mix kernel's 0,4,1,5,... order; "
                                        "Ap = 8 > A; tensors of 30 and 5 floats: padding in the flat buffers"),
    "tiles": (9, 65, 17, 4, 43, 3, 2, "129 rows: a second 128-row trip of the embedding wgrad and a fifth 32-row mix tile, "
                                      "one row each; H = 65: a one-column last block of the 64-column mix blocks and of the "
                                      "16-column wgrad blocks; E = 17: the same in the wgrad's feature blocks; Ap == A"),
    "wide": (7, 64, 128, 64, 5, 4, 4, "E = IQN_MAX_E and A = IQN_MAX_A: both LDS panels of the mix kernel full, every lane "
                                      "of the head's wave an action"),
    "fractions": (6, 32, 8, 33, 3, 70, 256, "N'' = IQN_MAX_TAU: four passes of the head's Bellman-target loop; N' = 70: two "
                                            "passes of its loss loop; A = 33: more actions than half a wave"),
}
RAGGED_ACTIONS = (1, 2, 4, 5, 8, 33, 63, 64)
KAPPAS = (0.5, 1.0)


def learn_case(shape, A=None, kappa=1.0, clip=False, tie=False):
    S, H, E, A0, B, NP, NPP, why = LEARN_SHAPES[shape]
    A = A0 if A is None else A
    covers = f"{why}; A = {A}, kappa = {kappa}; " + ("the gradient norm is past twice max_norm" if clip else "clipping inactive")
    if tie:
        covers += f"; rows {TIE_PAIR[0]} and {TIE_PAIR[1]} of value_net.2 identical: exact ties of the Double-DQN means"
    return dict(name=f"{shape}-a{A}-k{kappa}-{'clip' if clip else 'free'}" + ("-tie" if tie else ""), shape=shape, S=S, H=H,
                E=E, A=A, B=B, NP=NP, NPP=NPP, kappa=kappa, clip=clip, tie=tie, covers=covers)


# every shape with clipping inactive and active; on `ragged` the full A x kappa product; one designed tie
LEARN_CASES = {}
for _c in ([learn_case(s, clip=c) for s in LEARN_SHAPES for c in (False, True)]
           + [learn_case("ragged", A=a, kappa=k) for a, k in itertools.product(RAGGED_ACTIONS, KAPPAS)]
           + [learn_case("ragged", tie=True)]):
    LEARN_CASES.setdefault(_c["name"], _c)
LEARN_NAMES = list(LEARN_CASES)


def ru4(n):
    return (n + 3) // 4 * 4


def shapes_of(S, H, E, A):
    """Parameter shapes in IO.NAMES (= IQNNetwork.parameters()) order."""
    return [(H, S), (H,), (H, H), (H,), (H, E), (H,), (H, H), (H,), (A, H), (A,)]


def offsets_of(S, H, E, A):
    """(offsets, n_params) of engine.IqnEngine's flat layout: every tensor starts on a 16-byte boundary."""
    offs, off = [], 0
    for shp in shapes_of(S, H, E, A):
        offs.append(off)
        off += ru4(int(np.prod(shp)))
    return offs, off


def _net(rng, S, H, E, A, head_scale=1.4):
    P = {}
    for name, shp in zip(IO.NAMES, shapes_of(S, H, E, A)):
        if len(shp) == 2:
            scale = head_scale if name == "value_net.2.weight" else 1.4
            P[name] = (scale * rng.standard_normal(shp) / np.sqrt(shp[1])).astype(np.float32)
        else:
            P[name] = (0.1 * rng.standard_normal(shp)).astype(np.float32)
    return P


def preacts(P, states, taus):
    """fp64 pre-activations of the three ReLUs on (states, taus): (B, H), (B, H), (B, N, H)."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}
    states, taus = np.asarray(states, dtype=np.float64), np.asarray(taus, dtype=np.float64)
    z0 = states @ P["feature_net.0.weight"].T + P["feature_net.0.bias"]
    z1 = np.maximum(z0, 0.0) @ P["feature_net.2.weight"].T + P["feature_net.2.bias"]
    emb = IO.cos_embed(taus, P["quantile_embedding.weight"].shape[1]) @ P["quantile_embedding.weight"].T + P["quantile_embedding.bias"]
    zv = (np.maximum(z1, 0.0)[:, None, :] * emb) @ P["value_net.0.weight"].T + P["value_net.0.bias"]
    return z0, z1, zv


def mean_q(P, states, taus):
    """fp64 tau-mean of the network's output: (B, A)."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}
    return IO.forward(P, np.asarray(states, dtype=np.float64), np.asarray(taus, dtype=np.float64)).mean(1)


def top2_gap(q):
    if q.shape[1] < 2:
        return np.full(q.shape[0], np.inf)
    s = np.sort(q, axis=1)
    return s[:, -1] - s[:, -2]


def sample_margins(case, online, states, next_states, taus_p, taus_pp):
    """Per sample: (smallest |pre-activation| of the online net on (s, tau'), top-two gap of its tau''-mean on s',
    designed tie that is the maximum by MARGIN)."""
    z0, z1, zv = preacts(online, states, taus_p)
    B = states.shape[0]
    relu = np.minimum(np.minimum(np.abs(z0).min(1), np.abs(z1).min(1)), np.abs(zv).reshape(B, -1).min(1))
    q = mean_q(online, next_states, taus_pp)
    tie = np.zeros(B, dtype=bool)
    if case["tie"]:
        j1, j2 = TIE_PAIR
        tie = (q[:, j1] == q[:, j2]) & (q[:, j1] - np.delete(q, [j1, j2], axis=1).max(1) >= MARGIN)
    return relu, top2_gap(q), tie


def make_learn(case):
    S, H, E, A, B, NP, NPP = (case[k] for k in ("S", "H", "E", "A", "B", "NP", "NPP"))
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    online = _net(rng, S, H, E, A)
    N = 3 * B + 7                                        # more replay rows than the minibatch takes
    states = rng.standard_normal((N, S)).astype(np.float32)
    next_states = rng.standard_normal((N, S)).astype(np.float32)
    if case["tie"]:
        # both rows of the pair take the row that wins most often on s', so the pair is often the maximum
        k = np.bincount(mean_q(online, next_states, rng.random((N, NPP)).astype(np.float32)).argmax(1), minlength=A).argmax()
        w, b = online["value_net.2.weight"], online["value_net.2.bias"]
        if k not in TIE_PAIR:                            # row k changes places with the pair's first row: no third copy
            w[[k, TIE_PAIR[0]]], b[[k, TIE_PAIR[0]]] = w[[TIE_PAIR[0], k]], b[[TIE_PAIR[0], k]]
            k = TIE_PAIR[0]
        for j in TIE_PAIR:
            w[j], b[j] = w[k].copy(), b[k]
    target = {k: (v + 0.05 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in online.items()}
    actions = rng.integers(0, A, N).astype(np.int64)
    rewards = rng.standard_normal(N).astype(np.float32)
    dones = (rng.uniform(size=N) < 0.25).astype(np.float32)
    # Moments of a run in progress, as tests/helpers/qstep_cases.py draws them: |m| below ~2e-3, sqrt(v) >= 5e-3
    adam_m = {k: (5e-4 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in online.items()}
    adam_v = {k: ((0.01 * (0.5 + np.abs(rng.standard_normal(v.shape)))) ** 2).astype(np.float32) for k, v in online.items()}
    for _ in range(400):          # seeded redraws until the minibatch shows what the case is there to show
        idx, tp, tpp, ties = [], [], [], []
        for r in rng.permutation(N):
            for _try in range(8):                        # candidates: the row with fresh fractions
                a, b = rng.random((1, NP)).astype(np.float32), rng.random((1, NPP)).astype(np.float32)
                relu, gap, tie = sample_margins(case, online, states[r:r + 1], next_states[r:r + 1], a, b)
                if relu[0] >= MARGIN and (gap[0] >= MARGIN or tie[0]):
                    idx.append(r), tp.append(a[0]), tpp.append(b[0]), ties.append(bool(tie[0]))
                    break
            if len(idx) == B:
                break
        if len(idx) < B:
            continue
        idx, ties = np.array(idx, dtype=np.int64), np.array(ties)
        if (B > 1 and (np.diff(idx) > 0).all()) or (np.sort(idx) == np.arange(B)).all():
            continue                                     # neither sorted nor a prefix of the replay arrays
        if B >= 3 and len(np.unique(dones[idx])) < 2:
            continue
        if B < 3 and dones[idx].any():
            continue
        if case["tie"] and int((ties & (dones[idx] == 0)).sum()) < 3:
            continue
        break
    else:
        raise ValueError(f"{case['name']}: no admissible minibatch")
    d = dict(case=case, online=online, target=target, states=states, next_states=next_states, actions=actions, rewards=rewards,
             dones=dones, adam_m=adam_m, adam_v=adam_v, idx=idx, taus_prime=np.stack(tp), taus_dprime=np.stack(tpp),
             tie_samples=ties, n_rows=N, max_norm=1e30)
    total = learn_step(d, np.float64)["norm"]            # the fp64 gradient norm decides max_norm
    d["max_norm"] = float(np.float32(total / 3.0 if case["clip"] else max(10.0, 4.0 * total)))
    assert total > 2.0 * d["max_norm"] if case["clip"] else total + 1e-6 < d["max_norm"], (case["name"], total, d["max_norm"])
    return d


def learn_step(d, dtype):
    """One IQNTrainer.learn step of the case by oracle/iqn_oracle.IqnOracle in `dtype`."""
    c, i = d["case"], d["idx"]
    o = IO.IqnOracle(d["online"], d["target"], gamma=GAMMA, kappa=c["kappa"], lr=LR, max_norm=d["max_norm"], dtype=dtype,
                     m=d["adam_m"], v=d["adam_v"], t=STEP - 1)
    loss = o.learn(d["states"][i], d["actions"][i], d["rewards"][i], d["next_states"][i], d["dones"][i], d["taus_prime"],
                   d["taus_dprime"])
    return dict(loss=loss, norm=float(o.grad_norm), coef=float(o.coef), grads=[o.G[k] for k in IO.NAMES], a_star=o.a_star,
                params=[o.P[k] for k in IO.NAMES], adam_m=[o.m[k] for k in IO.NAMES], adam_v=[o.v[k] for k in IO.NAMES])


def step64(d):
    return learn_step(d, np.float64)


def step32(d):
    """The control that sets the GPU bars: the same class in float32, numpy's summation orders."""
    return learn_step(d, np.float32)


def grad_scale(g64):
    s = float(np.abs(g64).max())
    return s if s > 0.0 else 1.0


STAT_NAMES = ("loss", "norm", "coef")


def learn_errors(ref64, got):
    """Error of `got` (the control, or a device result with the same keys) against the fp64 step: loss, total norm and clip
    coefficient as relative errors, each gradient tensor as its largest absolute error over its own fp64 max-abs."""
    e = {k: abs(float(got[k]) - ref64[k]) / abs(ref64[k]) for k in STAT_NAMES}
    e["grads"] = [float(np.abs(np.asarray(g, dtype=np.float64) - g64).max() / grad_scale(g64))
                  for g, g64 in zip(got["grads"], ref64["grads"])]
    return e


def adam64(params, grads, m, v, step=STEP, lr=LR, betas=BETAS, eps=EPS):
    """torch.optim.Adam's update (no weight decay, no amsgrad) in fp64 on arrays of any one shape -> (params, m, v)."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (params, grads, m, v))
    b1, b2 = betas
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * m / denom, m, v


# selectors that mirror the kernels' conditions (csrc/iqn.hpp, csrc/iqn_api.inc)
def sel_vec(H):
    """iqn_act_head_kernel reads 16 bytes at a time (the flat buffers and the workspace are 16-byte aligned)."""
    return H % 4 == 0


def sel_wgrad_trips(rows):
    """(trips of iqn_embed_wgrad_kernel's 128-row staging loop, rows of the last one)."""
    return -(-rows // WG_ROWS), (rows - 1) % WG_ROWS + 1


def sel_mix_tiles(rows):
    return -(-rows // MIX_ROWS), (rows - 1) % MIX_ROWS + 1


def sel_last_block(n, block):
    """Columns of the last block when n columns are split into blocks of `block`."""
    return (n - 1) % block + 1


def sel_lane_passes(n):
    """Trips of a `for (i = lane; i < n; i += 64)` loop."""
    return -(-n // 64)


def sel_act_threads(n_tau):
    return 1024 if n_tau >= 16 else 256


# ---- act cases ------------------------------------------------------------------------------------------------------
ACT2_S, ACT2_E, ACT2_STATES = 7, 10, 16
ACT_GRID = [(H, n, A) for H in (30, 32) for n in (1, 15, 16, 17, 256) for A in (1, 5, 64)]
ACT_PROBES = [(probe, H, n) for probe in ("lastk", "nan1", "nan2", "target") for H in (30, 32) for n in (3, 17)]
ACT_PROBE_A = 5


def _act_states(rng, P, n_tau, A, accept, distinct):
    """ACT2_STATES states with fractions, every one decided (fp64 top-two gap >= ACT_MIN_GAP) and accepted by `accept(q)`,
    their answers taking at least `distinct` values: slots are kept back for answers not seen yet."""
    states, taus, seen = [], [], set()
    for _ in range(400):
        cs = (1.5 * rng.standard_normal((64, ACT2_S))).astype(np.float32)
        ct = rng.random((64, n_tau)).astype(np.float32)
        q = mean_q(P, cs, ct)
        ok = (top2_gap(q) >= ACT_MIN_GAP) & accept(cs, ct, q)
        for i in np.flatnonzero(ok):
            a = int(np.argmax(q[i]))
            if a in seen and ACT2_STATES - len(states) <= distinct - len(seen):
                continue
            seen.add(a), states.append(cs[i]), taus.append(ct[i])
            if len(states) == ACT2_STATES:
                return np.stack(states), np.stack(taus)
    raise ValueError("no admissible act states")


def act_grid_case(H, n_tau, A):
    """-> dict(P, states (16, S), taus (16, n_tau), want): a seeded network whose head spreads its answers."""
    rng = np.random.default_rng(zlib.crc32(f"act-{H}-{n_tau}-{A}".encode()))
    P = _net(rng, ACT2_S, H, ACT2_E, A, head_scale=4.0)
    # The hidden rows of the value net are non-negative, so each action's mean carries its head row times their average: a
    # constant that would give one action nearly every state.  The bias takes it away; the answer is left to the state.
    cs, ct = (1.5 * rng.standard_normal((256, ACT2_S))), rng.random((256, n_tau))
    v0 = IO.forward({k: v.astype(np.float64) for k, v in P.items()}, cs, ct, keep=True)[1][-1]
    P["value_net.2.bias"][:] = -(P["value_net.2.weight"].astype(np.float64) @ v0.mean((0, 1))).astype(np.float32)
    states, taus = _act_states(rng, P, n_tau, A, lambda cs, ct, q: np.ones(len(q), dtype=bool), min(A, 8))
    return dict(P=P, T=P, states=states, taus=taus, want=mean_q(P, states, taus).argmax(1), which=0)


def act_probe_case(probe, H, n_tau):
    """Designed probes of the act head, A = 5:
    lastk   value_net.2 reads only the last hidden unit k = H - 1 (the scalar tail of lane H - 1 when H = 30, the last
            float4 of lane 7 when H = 32); a head that misses it answers with its largest bias, which every state avoids
    nan1    value_net.2.bias holds NaN at action 2: the NaN wins
    nan2    NaN at actions 1 and 3: the first NaN wins
    target  which = 1: the answer of the target parameters, different from the online parameters' on every state"""
    A = ACT_PROBE_A
    rng = np.random.default_rng(zlib.crc32(f"probe-{probe}-{H}-{n_tau}".encode()))
    P = _net(rng, ACT2_S, H, ACT2_E, A, head_scale=4.0)
    P["value_net.2.bias"][:] = 0.0
    T, which, everything = P, 0, lambda cs, ct, q: np.ones(len(q), dtype=bool)
    if probe == "lastk":
        col = P["value_net.2.weight"][:, H - 1].copy()
        P["value_net.2.weight"][:] = 0.0
        P["value_net.2.weight"][:, H - 1] = 4.0 * col
        P["value_net.2.bias"][:] = (0.05 * rng.standard_normal(A)).astype(np.float32)
        P["value_net.0.bias"][H - 1] = 1.0                       # the unit the head reads is usually alive
        by_bias = int(np.argmax(P["value_net.2.bias"]))
        states, taus = _act_states(rng, P, n_tau, A, lambda cs, ct, q: q.argmax(1) != by_bias, 1)
        want = mean_q(P, states, taus).argmax(1)
    elif probe in ("nan1", "nan2"):
        states, taus = _act_states(rng, P, n_tau, A, everything, 1)
        where = (2,) if probe == "nan1" else (1, 3)
        assert not np.isin(mean_q(P, states, taus).argmax(1), where).all()      # the finite answer is another one somewhere
        for a in where:
            P["value_net.2.bias"][a] = np.nan
        want = np.full(ACT2_STATES, where[0])
    else:
        T = _net(rng, ACT2_S, H, ACT2_E, A, head_scale=4.0)
        T["value_net.2.bias"][:] = 0.0
        which = 1
        differs = lambda cs, ct, q: (top2_gap(mean_q(T, cs, ct)) >= ACT_MIN_GAP) & (mean_q(T, cs, ct).argmax(1) != q.argmax(1))
        states, taus = _act_states(rng, P, n_tau, A, differs, 1)
        want = mean_q(T, states, taus).argmax(1)
    return dict(P=P, T=T, states=states, taus=taus, want=want, which=which)
