"""IQN in the vectorised loop on the device (csrc/iqn_vector.hpp, the new entry points of csrc/iqn_api.inc,
train/vector_iqn.py), against the numpy restatements of tests/helpers/iqn_vector_cases.py, the fp64 oracle and the cases of
tests/helpers/iqn_cases.py.

  1. the fraction stream bit for bit against numpy;
  2. the rows head over a grid of K, A and ld: values bit-equal to the sequential fp32 sum, actions bit-equal to
     engine.qnet_select on the values written, NaN rules, values written when every robot explores;
  3. IqnEngine.act_rows against the fp64 oracle on ACT_GRID and the `target` probe;
  4. keyed fractions and chunking;
  5. learn_sampled against sample_indices + iqn_draw_taus + learn;
  6. train_vectorized_iqn against a hand-written loop, a rerun, a split run, another seed, and its refusals.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import iqn_cases as IC
from helpers import iqn_vector_cases as VC
from oracle import iqn_oracle as IO
from porl_amd import _native as N
from porl_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLOOR, CONTROL_FACTOR = 2e-6, 2.0                       # tests/test_iqn_engine_gpu.py's floor and factor
BUFFERS = ("params", "params_tgt", "grads", "adam_m", "adam_v")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _engine(S, A, Ed, H, max_batch, max_tau):
    eng = E.IqnEngine(S, A, Ed, H, max_batch, max_tau, DEV)
    bufs = {k: torch.zeros(eng.n_params, dtype=torch.float32, device=DEV) for k in BUFFERS}
    eng.bind(*[bufs[k] for k in BUFFERS])
    return eng, bufs


def _write(eng, flat, tensors):
    for name, off, shp in zip(IO.NAMES, eng.offsets, IC.shapes_of(eng.cfg.state_dim, eng.cfg.hidden, eng.cfg.embedding_dim,
                                                                  eng.cfg.n_actions)):
        t = _dev(np.asarray(tensors[name], dtype=np.float32))
        assert tuple(t.shape) == tuple(shp)
        flat[off:off + t.numel()].copy_(t.reshape(-1))


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


# ---- 1. the stream -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use", [0, 1, 2])
def test_draw_taus_is_the_numpy_stream(use):
    seed, draw = 0xC0FFEE12345, 77
    for first in (0, 4099):
        for count in (1, 63, 64, 65, 1000):
            got = E.iqn_draw_taus(seed, use, draw, first, count, device=DEV).cpu().numpy()
            assert got.tobytes() == VC.taus(seed, use, draw, first, count).tobytes(), (first, count)
    whole = E.iqn_draw_taus(seed, use, draw, 5, 1000, device=DEV)
    halves = torch.cat([E.iqn_draw_taus(seed, use, draw, 5, 500, device=DEV), E.iqn_draw_taus(seed, use, draw, 505, 500, device=DEV)])
    assert torch.equal(whole, halves)
    # the top of both ranges
    top = E.iqn_draw_taus(seed, use, (1 << 32) - 1, (1 << 32) - 7, 7, device=DEV).cpu().numpy()
    assert top.tobytes() == VC.taus(seed, use, (1 << 32) - 1, (1 << 32) - 7, 7).tobytes()
    out = torch.zeros(8, dtype=torch.float32, device=DEV)
    E.iqn_draw_taus(seed, use, draw, 3, 5, out=out[1:6])                   # an output off the 16-byte grid
    assert out[0] == 0 and (out[6:] == 0).all() and out[1:6].cpu().numpy().tobytes() == VC.taus(seed, use, draw, 3, 5).tobytes()


# ---- 2. the rows head ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("A", VC.HEAD_A)
@pytest.mark.parametrize("K", VC.HEAD_K)
def test_select_rows_grid(K, A, pad):
    zh = VC.head_z(K, A, pad)
    n, seed, t, off = VC.HEAD_N, 99, 12, 40
    want = VC.mean_rows_f32(zh[:, :A], K)
    z = _dev(zh)
    assert z.stride(0) == (A + 3) // 4 * 4 + pad
    for eps in (0.0, 0.3, 1.0):
        table = torch.full((n, A + 3), float("nan"), dtype=torch.float32, device=DEV)
        q = table[:, 1:1 + A]
        acts = E.iqn_select_rows(z[:, :A], K, eps, seed, t, env_offset=off, q=q)
        got = q.cpu().numpy()
        assert got.tobytes() == want.tobytes(), f"eps {eps}: values differ from the sequential fp32 sum"     # also at eps = 1
        assert bool(torch.isnan(table[:, 0]).all()) and bool(torch.isnan(table[:, 1 + A:]).all())
        ref = E.qnet_select(q.contiguous(), eps, seed, t, env_offset=off)
        assert torch.equal(acts, ref), f"eps {eps}"
        if eps == 0.0 and A > 1:
            assert np.array_equal(acts.cpu().numpy(), want.argmax(1))
    if A > 1:
        assert not torch.equal(acts, E.iqn_select_rows(z[:, :A], K, 0.0, seed, t, env_offset=off))        # eps = 1 explored


@pytest.mark.parametrize("vec", [True, False])
def test_select_rows_nan_rules_and_unaligned_rows(vec):
    """One NaN action wins; of two the first wins (the rule of tests/test_iqn_engine_gpu.py's nan1 / nan2 probes); a table
    off the 16-byte grid with ld = 7 takes the float-by-float staging and gives the same bits."""
    K, A, n = 17, 5, 9
    rng = np.random.default_rng(5)
    base = rng.standard_normal((n * K, A)).astype(np.float32)
    ld = 8 if vec else 7
    store = torch.full((n * K * ld + 1,), float("nan"), dtype=torch.float32, device=DEV)
    z = store[0 if vec else 1:][:n * K * ld].view(n * K, ld)[:, :A]
    for where, answer in (((), None), ((2,), 2), ((1, 3), 1)):
        zh = base.copy()
        for a in where:
            zh[np.arange(n) * K + (np.arange(n) % K), a] = np.nan        # one fraction of the action is NaN: so is its mean
        z.copy_(_dev(zh))
        q = torch.empty(n, A, dtype=torch.float32, device=DEV)
        acts = E.iqn_select_rows(z, K, 0.0, 1, 0, q=q).cpu().numpy()
        want = VC.mean_rows_f32(zh, K)
        assert np.array_equal(np.isnan(q.cpu().numpy()), np.isnan(want))
        assert np.nan_to_num(q.cpu().numpy()).tobytes() == np.nan_to_num(want).tobytes()
        assert np.array_equal(acts, want.argmax(1) if answer is None else np.full(n, answer))


# ---- 3. act against fp64 -------------------------------------------------------------------------------------------------
ACT_IDS = [("grid",) + k for k in IC.ACT_GRID] + [("probe",) + k for k in IC.ACT_PROBES if k[0] == "target"]


@functools.lru_cache(maxsize=None)
def _act_ref(key):
    """(case, fp64 mean_q, the fp32 control's error relative to the largest |q|) — computed once, never modified."""
    c = IC.act_grid_case(*key[1:]) if key[0] == "grid" else IC.act_probe_case(*key[1:])
    P = c["T"] if c["which"] else c["P"]
    q64 = IC.mean_q(P, c["states"], c["taus"])
    P32 = {k: np.asarray(v, dtype=np.float32) for k, v in P.items()}
    q32 = IO.forward(P32, c["states"].astype(np.float32), c["taus"].astype(np.float32)).mean(1)
    assert q32.dtype == np.float32
    scale = float(np.abs(q64).max())
    return c, q64, scale, float(np.abs(q32.astype(np.float64) - q64).max() / scale)


@pytest.mark.parametrize("key", ACT_IDS, ids=lambda k: "-".join(map(str, k)))
def test_act_rows_matches_the_fp64_oracle(key):
    """Every row of every case answers with the oracle's action (none is skipped) and its A values lie within
    max(2e-6, 2 x the fp32 control's error) of the fp64 tau-mean, relative to the case's largest |q|.

    Largest measured error / bar over the 34 cases (MI355X), q: 0.51 (grid H = 30, K = 15, A = 5: 1.0e-6 of the 2e-6
    floor); the one case whose bar is above the floor is grid H = 32, K = 1, A = 5 (2.2e-6, ratio 0.48).  The actions
    matched on every row.  The figure of each case is printed before the assertion."""
    c, q64, scale, control = _act_ref(key)
    H, n_tau = (key[1], key[2]) if key[0] == "grid" else (key[2], key[3])
    A, S = c["P"]["value_net.2.bias"].shape[0], IC.ACT2_S
    n = len(c["states"])
    eng, bufs = _engine(S, A, IC.ACT2_E, H, n, n_tau)
    _write(eng, bufs["params"], c["P"])
    if c["which"]:
        _write(eng, bufs["params_tgt"], c["T"])
    else:
        bufs["params_tgt"].fill_(float("nan"))                # which = 0 reads nothing of the target parameters
    eng.workspace.fill_(float("nan"))
    wide = torch.full((n, S + 3), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, :S] = _dev(c["states"])
    states, taus = wide[:, :S], _dev(c["taus"])
    assert states.stride(0) == S + 3
    q = torch.empty(n, A, dtype=torch.float32, device=DEV)
    acts = eng.act_rows(states, n_tau, 0.0, 1, 0, taus=taus, q=q, which=c["which"])
    rec = torch.full((n, 16), -1, dtype=torch.int32, device=DEV)
    for i in range(n):
        eng.act(rec[i], taus[i:i + 1], states=states, row=i, which=c["which"], n_stats=0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(acts.cpu().numpy(), c["want"], err_msg="act_rows against the oracle")
    np.testing.assert_array_equal(rec[:, 0].cpu().numpy(), c["want"], err_msg="porl_iqn_act on the same rows")
    err = float(np.abs(q.cpu().numpy().astype(np.float64) - q64).max() / scale)
    bar = max(FLOOR, CONTROL_FACTOR * control)
    print(f"\n[iqn-vector] act {'-'.join(map(str, key))} | err {err:.3g} bar {bar:.3g} ratio {err / bar:.3f}")
    assert err <= bar, f"q: error {err:.3g} > bar {bar:.3g}"


# ---- 4. keyed and chunked ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_offset", [0, 1000])
def test_act_rows_keyed_fractions_and_chunks(env_offset):
    """taus=None is act_rows on the stream's elements [(env_offset) * n_tau, (env_offset + n) * n_tau) of use 0 at draw t,
    bit for bit in q and actions, at n = 1, 4, 5, 9 on an engine of max_batch = 4 (chunks 4, 4, 1); robots [3, 9) run alone
    with env_offset + 3 repeat their rows of the full run.

    The bits of q across chunkings ARE required equal here: every product of these shapes has K <= 128, where pick_tile
    returns TILE_64x64 whatever M is, and inside one tile shape an output element is one accumulator's chain over k, which a
    row's position in the chunk does not enter.  For K > 128 pick_tile's choice depends on M and nothing is claimed."""
    S, A, Ed, H, n_tau, seed, t = IC.ACT2_S, 5, IC.ACT2_E, 30, 7, 31337, 5
    rng = np.random.default_rng(17)
    eng, bufs = _engine(S, A, Ed, H, 4, n_tau)
    _write(eng, bufs["params"], IC._net(rng, S, H, Ed, A, head_scale=4.0))
    bufs["params_tgt"].fill_(float("nan"))
    states = _dev((1.5 * rng.standard_normal((9, S))).astype(np.float32))
    full = None
    for n in (1, 4, 5, 9):
        eng.workspace.fill_(float("nan"))
        q1, q2 = (torch.empty(n, A, dtype=torch.float32, device=DEV) for _ in range(2))
        a1 = eng.act_rows(states[:n], n_tau, 0.3, seed, t, env_offset=env_offset, q=q1)
        T = E.iqn_draw_taus(seed, 0, t, env_offset * n_tau, n * n_tau, device=DEV).view(n, n_tau)
        assert T.cpu().numpy().tobytes() == VC.taus(seed, 0, t, env_offset * n_tau, n * n_tau).tobytes()
        eng.workspace.fill_(float("nan"))
        a2 = eng.act_rows(states[:n], n_tau, 0.3, seed, t, env_offset=env_offset, taus=T, q=q2)
        assert torch.equal(a1, a2) and _bits(q1) == _bits(q2), n
        assert bool(torch.isfinite(q1).all())
        assert torch.equal(a1, E.qnet_select(q1, 0.3, seed, t, env_offset=env_offset))
        full = (a1, q1)
    qt = torch.empty(6, A, dtype=torch.float32, device=DEV)
    tail = eng.act_rows(states[3:9], n_tau, 0.3, seed, t, env_offset=env_offset + 3, q=qt)
    assert torch.equal(tail, full[0][3:9])
    assert _bits(qt) == _bits(full[1][3:9])
    q3 = torch.empty(9, A, dtype=torch.float32, device=DEV)
    eng.act_rows(states, n_tau, 0.3, seed, t + 1, env_offset=env_offset, q=q3)
    assert _bits(q3) != _bits(full[1])                          # another act-step draws other fractions


# ---- 5. the sampled learn step -------------------------------------------------------------------------------------------
def _learn_pair(B, NP, NPP, max_batch):
    S, A, Ed, H = IC.ACT2_S, 5, IC.ACT2_E, 30
    rng = np.random.default_rng(1000 * B + NP)
    online = IC._net(rng, S, H, Ed, A)
    target = {k: (v + 0.05 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in online.items()}
    m = {k: (5e-4 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in online.items()}
    v = {k: ((0.01 * (0.5 + np.abs(rng.standard_normal(v_.shape)))) ** 2).astype(np.float32) for k, v_ in online.items()}
    pair = []
    for _ in range(2):
        eng, bufs = _engine(S, A, Ed, H, max_batch, max(NP, NPP))
        for k, src in (("params", online), ("params_tgt", target), ("adam_m", m), ("adam_v", v)):
            _write(eng, bufs[k], src)
        eng.workspace.fill_(float("nan"))
        pair.append((eng, bufs))
    rows = 100
    replay = [_dev(rng.standard_normal((rows, S)).astype(np.float32)), _dev(rng.integers(0, A, rows).astype(np.int64)),
              _dev(rng.standard_normal(rows).astype(np.float32)), _dev(rng.standard_normal((rows, S)).astype(np.float32)),
              _dev((rng.uniform(size=rows) < 0.25).astype(np.float32))]
    return pair, replay


@pytest.mark.parametrize("NP,NPP", [(8, 8), (3, 65)])
@pytest.mark.parametrize("B", [1, 5, 32])
def test_learn_sampled_is_sample_indices_draw_taus_and_learn(B, NP, NPP):
    seed = 4242
    for n_rows in (B, 100):
        ((ea, ba), (eb, bb)), replay = _learn_pair(B, NP, NPP, 32)
        for draw in (6, 7):                                    # two successive draws
            step = draw - 5
            hp = ea.hyper(0.97, 1.0, 10.0, step, 5e-4)
            assert ea.learn_sampled(hp, *replay, n_rows, B, seed, draw, NP, NPP) == B
            idx = E.sample_indices(n_rows, B, seed, draw, device=DEV)
            tp = E.iqn_draw_taus(seed, 1, draw, 0, B * NP, device=DEV).view(B, NP)
            tpp = E.iqn_draw_taus(seed, 2, draw, 0, B * NPP, device=DEV).view(B, NPP)
            eb.learn(eb.hyper(0.97, 1.0, 10.0, step, 5e-4), *replay, idx, tp, tpp)
            for k in BUFFERS:
                assert _bits(ba[k]) == _bits(bb[k]), (n_rows, draw, k)
            assert _bits(ea.stats[:3]) == _bits(eb.stats[:3]) and bool(torch.isfinite(ea.stats[:3]).all())
        assert not torch.equal(ba["params"], torch.zeros_like(ba["params"]))


def test_learn_sampled_refused_leaves_every_buffer_alone():
    ((ea, ba), _), replay = _learn_pair(5, 8, 8, 8)
    ea.workspace.fill_(1.5)
    before = {k: v.clone() for k, v in ba.items()}
    stats = ea.stats.clone()
    hp = ea.hyper(0.97, 1.0, 10.0, 1, 5e-4)
    with pytest.raises(N.NativeError, match="n_rows"):
        ea.learn_sampled(hp, *replay, 4, 5, 1, 0, 8, 8)
    with pytest.raises(N.NativeError, match="batch"):
        ea.learn_sampled(hp, *replay, 100, 9, 1, 0, 8, 8)
    with pytest.raises(N.NativeError, match="draw"):
        ea.learn_sampled(hp, *replay, 100, 5, 1, 1 << 32, 8, 8)
    torch.cuda.synchronize()
    for k in BUFFERS:
        assert torch.equal(ba[k], before[k]), k
    assert torch.equal(ea.stats, stats) and bool((ea.workspace == 1.5).all())


# ---- 6. the loop ---------------------------------------------------------------------------------------------------------
N_ENVS, N_BEAMS, S, A, B, H, STEPS, BLOCK, STARTS, LOOP_SEED = 8, 1, 3, 5, 4, 32, 12, 4, 8, 5


def make_sim(**kw):
    from porl_amd.env import DiscreteLidarNavSim, NavWorld
    kw = dict(dict(n_actions=A, seed=3, auto_reset=True, n_beams=N_BEAMS, episode_step=20), **kw)
    return DiscreteLidarNavSim(NavWorld.lattice(), N_ENVS, **kw)


def make_trainer(tmp_path, cls=None):
    from porl_amd.train.iqn_trainer import IQNTrainer
    torch.manual_seed(11)
    return (cls or IQNTrainer)(S, A, 0.99, epsilon=1.0, epsilon_min=0.05, epsilon_decay=0.5, update_target_freq=1, device=DEV,
                               batch_size=B, embedding_dim=10, hidden_size=H, num_quantiles_n_policy=6,
                               num_quantiles_n_prime_loss=3, num_quantiles_n_double_prime_loss=5, buffer_size=64,
                               log_dir=str(tmp_path))


def run(tmp_path, n_steps=STEPS, seed=LOOP_SEED, calls=1):
    from porl_amd.buffer.device_replay import DeviceReplay
    t, sim = make_trainer(tmp_path), make_sim()
    replay = DeviceReplay(80, S, DEV)                           # 8 * 12 = 96 rows: the ring wraps
    outs = [t.train_vectorized_iqn(sim, n_steps // calls, replay=replay, learn_per_step=1, learning_starts=STARTS, block=BLOCK,
                                   seed=seed) for _ in range(calls)]
    return t, sim, replay, outs


def snapshot(t, sim, replay):
    o = t.optimizer
    return [x.clone() for x in (o.flat, t._target.flat, o.exp_avg, o.exp_avg_sq, sim.state, sim.counters, sim.obs,
                                sim.tallies, *replay.arrays())]


def assert_same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y) or (torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))), k


def hand_written(tmp_path):
    """The same steps from act_rows, sim.step(replay=...), learn_sampled and end_of_step."""
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.train.vector_online import end_of_step
    t, sim = make_trainer(tmp_path), make_sim()
    eng = t._native_engine(batch=max(B, N_ENVS))
    replay = DeviceReplay(80, S, DEV)
    sim.reset()
    acts = torch.empty(N_ENVS, dtype=torch.int64, device=DEV)
    losses, draw = [], 0
    for it in range(STEPS):
        eng.act_rows(sim.obs, 6, t.epsilon, LOOP_SEED, it, env_offset=sim.env_offset, out=acts)
        sim.step(acts, replay=replay)
        if len(replay) >= STARTS:
            hp = eng.hyper(t.gamma, t.kappa, t.max_norm, t.optimizer.step_count + 1, 5e-4)
            eng.learn_sampled(hp, *replay.arrays(), len(replay), B, LOOP_SEED, draw, 3, 5)
            t.optimizer.step_count = hp.step
            draw += 1
            losses.append(eng.stats[:1].clone())
        end_of_step(t, it, BLOCK)
    return t, sim, replay, torch.cat(losses).cpu().numpy()


def test_vectorized_training(tmp_path):
    t, sim, replay, (out,) = run(tmp_path)
    assert out["transitions"] == N_ENVS * STEPS == 96
    assert out["learn_steps"] == STEPS == t.optimizer.step_count == len(out["losses"]) == t._draws
    assert np.isfinite(out["losses"]).all() and (out["losses"] > 0).any()
    assert len(replay) == 80 and replay.position == 96 % 80 and t._vec_steps == STEPS
    assert t.epsilon == 0.125                                   # three blocks of decay 0.5
    assert (out["tallies"] == sim.tallies.sum(0).cpu().numpy()).all()
    fresh = make_trainer(tmp_path)
    assert not torch.equal(fresh.optimizer.flat, t.optimizer.flat) and bool(torch.isfinite(t.optimizer.flat).all())
    assert torch.equal(t.optimizer.flat, t._target.flat)        # update_target_freq = 1: synchronised after the last block
    # a rerun from a fresh trainer with the same seed
    t2, sim2, replay2, (out2,) = run(tmp_path)
    assert_same(snapshot(t, sim, replay), snapshot(t2, sim2, replay2))
    assert (out["losses"] == out2["losses"]).all() and (out["tallies"] == out2["tallies"]).all()
    # the hand-written loop
    t3, sim3, replay3, losses3 = hand_written(tmp_path)
    assert_same(snapshot(t, sim, replay), snapshot(t3, sim3, replay3))
    assert (out["losses"] == losses3).all()
    # one call of 12 steps equals two calls of 6
    t4, sim4, replay4, (first, second) = run(tmp_path, calls=2)
    assert_same(snapshot(t, sim, replay), snapshot(t4, sim4, replay4))
    assert (np.concatenate([first["losses"], second["losses"]]) == out["losses"]).all()
    assert first["learn_steps"] + second["learn_steps"] == STEPS
    # another seed gives other actions
    t5, sim5, replay5, _ = run(tmp_path, seed=LOOP_SEED + 1)
    assert not torch.equal(replay5.arrays()[1], replay.arrays()[1])


def test_default_learning_starts_is_training_learning_step(tmp_path):
    t = make_trainer(tmp_path)
    t.training_learning_step = 16
    assert t.train_vectorized_iqn(make_sim(), 3)["learn_steps"] == 2
    assert t.device_replay.capacity == 64 and len(t.device_replay) == 24


def test_refusals(tmp_path):
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.train.dqn_trainer import DQNTrainer
    from porl_amd.train.iqn_trainer import IQNTrainer
    from porl_amd.train.vector_online import train_vectorized_iqn
    sim = make_sim()
    sim_before = [x.clone() for x in (sim.state, sim.counters, sim.obs, sim.tallies)]
    dqn = DQNTrainer(S, A, 0.99, device=DEV, batch_size=B, log_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="the loop of IQNTrainer"):
        train_vectorized_iqn(dqn, sim, 4)
    assert dqn.optimizer.step_count == 0 and not hasattr(dqn, "_vec_steps")

    class Acts(IQNTrainer):
        def select_action(self, state):
            return 0

    class Learns(IQNTrainer):
        def learn_on(self, *batch, **kw):
            return super().learn_on(*batch, **kw)

    class LearnsWhole(IQNTrainer):
        def learn(self):
            return super().learn()

    for cls in (Acts, Learns, LearnsWhole):
        sub = make_trainer(tmp_path, cls=cls)
        with pytest.raises(NotImplementedError, match=r"train_online\(Env\("):
            sub.train_vectorized_iqn(sim, 4)
        assert sub.optimizer.step_count == 0 and not hasattr(sub, "_vec_steps")
    t = make_trainer(tmp_path)
    replay = DeviceReplay(100, S, DEV)
    with pytest.raises(ValueError, match="auto_reset"):
        t.train_vectorized_iqn(make_sim(auto_reset=False), 4, replay=replay)
    with pytest.raises(ValueError, match="observes"):
        t.train_vectorized_iqn(make_sim(n_beams=20), 4, replay=replay)
    with pytest.raises(ValueError, match="observes"):
        t.train_vectorized_iqn(make_sim(n_actions=4), 4, replay=replay)
    with pytest.raises(ValueError, match="learning_starts"):
        t.train_vectorized_iqn(sim, 4, replay=replay, learning_starts=101)
    with pytest.raises(ValueError, match="positive"):
        t.train_vectorized_iqn(sim, 0, replay=replay)
    off = make_trainer(tmp_path)
    w = off.q_network.value_net[2].weight
    w.data = w.data.clone()                                     # a parameter off the flat buffer
    with pytest.raises(RuntimeError, match="flat buffers"):
        off.train_vectorized_iqn(sim, 4, replay=replay)
    for tr in (t, off):
        assert tr.optimizer.step_count == 0 and not hasattr(tr, "_vec_steps") and not hasattr(tr, "device_replay")
    assert len(replay) == 0 and replay.position == 0
    for x, y in zip(sim_before, (sim.state, sim.counters, sim.obs, sim.tallies)):
        assert torch.equal(x, y) or torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
    tgt = make_trainer(tmp_path)
    fine = tgt.train_vectorized_iqn(sim, 1, replay=replay, learning_starts=8)       # and the same objects then run
    assert fine["transitions"] == N_ENVS and fine["learn_steps"] == 1
