"""C51 and QR-DQN in the vectorised loop (porl_amd/train/vector_dist.py) on the device: porl_dist_select against the fp64
oracle and the fp32 restatement of tests/helpers/dist_vector_cases.py, act_rows_dist against the chunked forward,
dist_learn_sampled against sample_indices + dist_learn, and the loop itself in test_vector_online_gpu.py's setting.

The only tolerance is C51's action values against the fp64 oracle: 8 x the restatement's own maximum error against the
oracle on the same logits (computed here, on the CPU; <= 5.7e-6 x 8 on the helper's grid) — the factor covers a device
expf / logf that is allowed an ulp or two more than numpy's — and the bar is asserted to stay below 1e-4, an order under
the 1e-3 gap that decides which rows are asked for their arg-max.  Measured on an MI355X over the grid: the worst
|device - oracle| was 5.7e-6 against its bar of 4.5e-5 (C51 (64, 4) at sigma 3).  Everything else is an identity."""
import functools

import numpy as np
import pytest
import torch

from helpers import dist_vector_cases as VC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 11


def head_of(kind, A, NS, support=None):
    from porl_amd import _native as N
    if kind == VC.C51:
        return N.DistHead(1, A, NS, 0.0, -VC.V_MAX, VC.V_MAX, support.data_ptr())
    return N.DistHead(0, A, NS, 1.0, 0.0, 0.0, None)


@functools.lru_cache(maxsize=None)
def reference(kind, A, NS, sigma):
    """Logits, support, fp64 oracle, fp32 restatement and top-2 gap of one case: computed once, never written to."""
    z = VC.logits(kind, A, NS, sigma)
    support = torch.linspace(-VC.V_MAX, VC.V_MAX, NS) if kind == VC.C51 else None
    sup = None if support is None else support.numpy()
    want = VC.oracle(kind, z, A, NS, sup)
    rest = VC.values_f32(kind, z, A, NS, sup)
    for x in (z, want, rest):
        x.setflags(write=False)
    return z, support, want, rest, VC.top2_gap(want)


def padded(z, pad=3):
    """z on the device with `pad` NaN columns behind every row: a row stride above the row width."""
    wide = torch.full((z.shape[0], z.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, :z.shape[1]] = torch.tensor(z).to(DEV)             # (a copy: the shared reference is read-only)
    return wide[:, :z.shape[1]]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def check_values(kind, got_q, want, rest, where):
    if kind == VC.QR:
        assert np.array_equal(bits(got_q), bits(rest)), where                     # (b) bit for bit
        return
    bar = 8.0 * float(np.abs(rest.astype(np.float64) - want).max())
    err = float(np.abs(got_q.astype(np.float64) - want).max())
    print(f"{where}: C51 max |device - oracle| {err:.3e}, bar {bar:.3e}")
    assert bar < 1e-4
    assert err <= bar, (where, err, bar)                                          # (c)


@pytest.mark.parametrize("kind,A,NS,sigma", VC.cases())
def test_dist_select_over_the_grid(kind, A, NS, sigma):
    from porl_amd.engine import dist_select, qnet_select
    z, support, want, rest, gap = reference(kind, A, NS, sigma)
    n = z.shape[0]
    assert n == 1029
    sup_dev = None if support is None else support.to(DEV)
    head = head_of(kind, A, NS, sup_dev)
    zd = padded(z)
    assert zd.stride(0) == A * NS + 3
    first = None
    for eps in (0.0, 0.3, 1.0):
        for t in (0, 9):
            table = torch.full((n, A + 2), float("nan"), dtype=torch.float32, device=DEV)
            q = table[:, 1:A + 1]
            out = dist_select(zd, head, eps, SEED, t, env_offset=2, q=q)
            assert out.dtype == torch.int64 and out.shape == (n,) and out.device.type == "cuda"
            assert bool(torch.isnan(table[:, 0]).all()) and bool(torch.isnan(table[:, A + 1]).all())      # (e)
            assert torch.equal(out, qnet_select(q, eps, SEED, t, env_offset=2)), (eps, t)                  # (a)
            got_q = q.cpu().numpy()
            if first is None:
                first = got_q
                check_values(kind, got_q, want, rest, f"kind {kind} ({A}, {NS}) sigma {sigma}")
            else:
                assert np.array_equal(bits(got_q), bits(first)), (eps, t)         # the values are written every time
            if eps == 0.0:                                                        # (d)
                far = gap >= VC.GAP
                assert np.array_equal(out.cpu().numpy()[far], want.argmax(axis=1)[far])
                assert torch.equal(out, torch.argmax(q, dim=1))
            if eps == 1.0 and t == 0:
                assert set(out.cpu().numpy().tolist()) == set(range(A))           # every action is explored
    # one run over the rows equals two runs over its halves with env_offset shifted
    both = dist_select(zd, head, 0.3, 4, 9, env_offset=2)
    assert torch.equal(both[:500], dist_select(zd[:500], head, 0.3, 4, 9, env_offset=2))
    assert torch.equal(both[500:], dist_select(zd[500:], head, 0.3, 4, 9, env_offset=502))
    # row counts around one block of four waves
    for m in (1, 3, 4, 5):
        qm = torch.full((m, A), float("nan"), dtype=torch.float32, device=DEV)
        om = dist_select(zd[:m], head, 0.3, SEED, 9, env_offset=2, q=qm)
        assert torch.equal(om, qnet_select(qm, 0.3, SEED, 9, env_offset=2)), m
        assert np.array_equal(bits(qm.cpu().numpy()), bits(first[:m])), m


@pytest.mark.parametrize("kind", [VC.QR, VC.C51])
def test_special_rows(kind):
    from porl_amd.engine import dist_select, qnet_select
    A, NS = 4, 70                                             # more than one element per lane
    rng = np.random.default_rng(3)
    z = rng.standard_normal((6, A, NS)).astype(np.float32)
    z[0, 1] += 2.0; z[0, 1, -5:] += 8.0                       # the best action under either head ...
    z[0, 3] = z[0, 1]                                         # ... twice, with identical columns: the lower index wins
    z[1, 2, 5] = np.nan                                       # a NaN value is the maximum
    z[2, 1, 69] = np.nan; z[2, 3, 0] = np.nan                 # the first of two NaNs wins
    z[3, 0] = z[3, 1] = z[3, 2] = z[3, 3]                     # all equal: action 0
    if kind == VC.QR:
        z[4, 2, 64] = np.inf                                  # a quantile at +inf: the mean is +inf
        z[5, 1, 3] = np.inf; z[5, 1, 4] = -np.inf             # inf - inf: NaN, which wins
    support = torch.linspace(-VC.V_MAX, VC.V_MAX, NS, device=DEV)
    head = head_of(kind, A, NS, support)
    q = torch.full((6, A), float("nan"), dtype=torch.float32, device=DEV)
    out = dist_select(torch.from_numpy(z.reshape(6, A * NS)).to(DEV), head, 0.0, SEED, 0, q=q)
    assert torch.equal(out, qnet_select(q, 0.0, SEED, 0))
    got, qv = out.cpu().numpy(), q.cpu().numpy()
    assert got[0] == 1 and bits(qv[0, 1]) == bits(qv[0, 3]) and qv[0, 1] > max(qv[0, 0], qv[0, 2])
    assert got[1] == 2 and np.isnan(qv[1, 2]) and not np.isnan(qv[1, [0, 1, 3]]).any()
    assert got[2] == 1 and np.isnan(qv[2, 1]) and np.isnan(qv[2, 3])
    assert got[3] == 0 and len(set(bits(qv[3]).tolist())) == 1
    if kind == VC.QR:
        assert got[4] == 2 and qv[4, 2] == np.inf
        assert got[5] == 1 and np.isnan(qv[5, 1])


# ---- the engine's two calls -------------------------------------------------------------------------------------------------
def make_trainer(kind, tmp_path, cls=None, batch=32, max_batch=4096, S=38, A=5, **kw):
    from porl_amd.train.c51_trainer import C51Trainer
    from porl_amd.train.qr_dqn_trainer import QRDQNTrainer
    torch.manual_seed(0)
    kw = dict(dict(epsilon=1.0, epsilon_min=0.05, epsilon_decay=0.5, update_target_freq=2, device=DEV, batch_size=batch,
                   max_batch=max_batch, log_dir=str(tmp_path), network_hidden_sizes=[64, 64]), **kw)
    if kind == "c51":
        return (cls or C51Trainer)(S, A, 0.99, atom_size=11, **kw)
    return (cls or QRDQNTrainer)(S, A, 0.99, num_quantiles=12, **kw)


@pytest.mark.parametrize("kind", ["c51", "qr"])
def test_act_rows_dist_equals_chunked_forward_then_dist_select(kind, tmp_path):
    """112 rows through an engine of max_batch 48: chunks of 48, 48 and 16."""
    from porl_amd.engine import dist_select
    t = make_trainer(kind, tmp_path, max_batch=48)
    eng, head = t._engine, t._dist_head()
    assert eng.cfg.max_batch == 48 and eng.cfg.n_actions == 5 * head.n_sub
    eng._ensure_bound()
    with torch.no_grad():
        eng.params_tgt.mul_(0.9)                              # a target network that differs (padding stays zero)
    obs = torch.randn(112, 38, device=DEV)
    tables = {}
    for which in (0, 1):
        for eps in (0.0, 0.4):
            want_q = torch.full((112, 5), float("nan"), device=DEV)
            want = torch.empty(112, dtype=torch.int64, device=DEV)
            for r in (0, 48, 96):
                zc = eng.forward(obs[r:r + 48], which=which)
                dist_select(zc, head, eps, 21, 6, env_offset=3 + r, q=want_q[r:r + 48], out=want[r:r + 48])
            table = torch.full((112, 7), float("nan"), device=DEV)
            got = eng.act_rows_dist(obs, head, eps, 21, 6, env_offset=3, q=table[:, 1:6], which=which)
            assert torch.equal(got, want) and torch.equal(table[:, 1:6], want_q), (which, eps)
            assert bool(torch.isnan(table[:, 0]).all()) and bool(torch.isnan(table[:, 6]).all())
            tables[which] = want_q
    assert not torch.equal(tables[0], tables[1])              # the two parameter sets were both exercised
    assert eng.act_rows_dist(obs, head, 0.0, 0, 0).shape == (112,)


def replay_rows(S, A, n=100):
    g = torch.Generator(device="cpu").manual_seed(9)
    return (torch.randn(n, S, generator=g).to(DEV), torch.randint(0, A, (n,), generator=g).to(DEV),
            (2.0 * torch.randn(n, generator=g)).to(DEV), torch.randn(n, S, generator=g).to(DEV),
            (torch.rand(n, generator=g) < 0.25).float().to(DEV))


@pytest.mark.parametrize("kind", ["c51", "qr"])
@pytest.mark.parametrize("B", [1, 5, 32])
def test_dist_learn_sampled_equals_sample_indices_then_dist_learn(kind, B, tmp_path):
    from porl_amd import engine as E
    rows = replay_rows(38, 5)
    for n_rows in (B, 100):
        ta, tb = make_trainer(kind, tmp_path), make_trainer(kind, tmp_path)
        ea, eb = ta._engine, tb._engine
        assert torch.equal(ea.params, eb.params)
        with torch.no_grad():
            for e in (ea, eb):
                e.params_tgt.mul_(0.9)
        for draw in (0, 1):
            hp = ta.optimizer.hyper(ta.gamma, 0.0, 1.0 / B)
            ea.dist_learn_sampled(hp, *rows, n_rows, B, SEED, draw, ta._dist_head())
            ta.optimizer.step_count = hp.step
            idx = E.sample_indices(n_rows, B, SEED, draw, device=eb.device)
            hp = tb.optimizer.hyper(tb.gamma, 0.0, 1.0 / B)
            eb.dist_learn(hp, *rows, idx, tb._dist_head())
            tb.optimizer.step_count = hp.step
            for name in ("params", "params_tgt", "adam_m", "adam_v"):
                assert torch.equal(getattr(ea, name), getattr(eb, name)), (n_rows, draw, name)
            assert torch.equal(ea.stats[:1], eb.stats[:1]) and bool(torch.isfinite(ea.stats[0]))
        assert ta.optimizer.step_count == 2 and not torch.equal(ea.params, make_trainer(kind, tmp_path)._engine.params)
    from porl_amd import _native as N
    with pytest.raises(N.NativeError, match="n_rows"):
        ea.dist_learn_sampled(ta.optimizer.hyper(ta.gamma, 0.0, 1.0 / B), *rows, B - 1, B, SEED, 0, ta._dist_head())


# ---- the loop -----------------------------------------------------------------------------------------------------------------
N_ENVS, N_BEAMS, S, A, B, STEPS, BLOCK, STARTS, LOOP_SEED = 64, 36, 38, 5, 32, 48, 16, 128, 5


def make_sim(**kw):
    from porl_amd.env import DiscreteLidarNavSim, NavWorld
    kw = dict(dict(n_actions=A, seed=3, auto_reset=True, n_beams=N_BEAMS, episode_step=20), **kw)
    return DiscreteLidarNavSim(NavWorld.lattice(), N_ENVS, **kw)


def run(kind, tmp_path, n_steps=STEPS):
    from porl_amd.buffer.device_replay import DeviceReplay
    t, sim = make_trainer(kind, tmp_path), make_sim()
    replay = DeviceReplay(2000, S, DEV)                         # 64 * 48 = 3072 rows: the ring wraps
    out = t.train_vectorized_dist(sim, n_steps, replay=replay, learn_per_step=1, learning_starts=STARTS, block=BLOCK, seed=LOOP_SEED)
    return t, sim, replay, out


def snapshot(t, sim, replay):
    eng = t._engine
    return [x.clone() for x in (eng.params, eng.params_tgt, eng.adam_m, eng.adam_v, sim.state, sim.counters, sim.obs,
                                sim.tallies, *replay.arrays())]


def assert_same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y) or (torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))), k


def hand_written(kind, tmp_path):
    """The same steps from the calls that existed before the sampled form: act_rows_dist -> step -> sample_indices +
    dist_learn, the block schedule on the host."""
    from porl_amd import engine as E
    from porl_amd.buffer.device_replay import DeviceReplay
    t, sim = make_trainer(kind, tmp_path), make_sim()
    eng, head = t._engine, t._dist_head()
    replay = DeviceReplay(2000, S, DEV)
    sim.reset()
    acts = torch.empty(N_ENVS, dtype=torch.int64, device=DEV)
    losses, draw, eps = [], 0, 1.0
    for it in range(STEPS):
        eng.act_rows_dist(sim.obs, head, eps, LOOP_SEED, it, env_offset=0, out=acts)
        sim.step(acts, replay=replay)
        if len(replay) >= STARTS:
            hp = t.optimizer.hyper(t.gamma, 0.0, 1.0 / B)
            idx = E.sample_indices(len(replay), B, LOOP_SEED, draw, device=eng.device)
            eng.dist_learn(hp, *replay.arrays(), idx, head)
            t.optimizer.step_count = hp.step
            draw += 1
            losses.append(eng.stats[:1].clone())
        if (it + 1) % BLOCK == 0:
            eps = max(0.05, eps * 0.5)
            if ((it + 1) // BLOCK - 1) % 2 == 0:
                t.sync_target()
    return t, sim, replay, torch.cat(losses).cpu().numpy()


@pytest.mark.parametrize("kind", ["c51", "qr"])
def test_vectorized_training(kind, tmp_path):
    from porl_amd.buffer.device_replay import DeviceReplay
    t, sim, replay, out = run(kind, tmp_path)
    eng = t._engine
    assert out["transitions"] == N_ENVS * STEPS == 3072
    assert out["learn_steps"] == STEPS - 1 == t.optimizer.step_count == len(out["losses"]) == t._draws
    assert bool(torch.isfinite(torch.from_numpy(out["losses"])).all()) and (out["losses"] > 0).any()
    assert len(replay) == 2000 and replay.position == 3072 % 2000 and t._vec_steps == STEPS
    assert t.epsilon == 0.125                                   # three blocks of decay 0.5
    tal = sim.tallies.sum(0).cpu().numpy()
    assert (out["tallies"] == tal).all() and 2 * N_ENVS <= tal[0] and tal[2] + tal[3] <= tal[0]
    # the parameters moved; the target network was synchronised after block 2 (b = 2, update_target_freq = 2)
    fresh = make_trainer(kind, tmp_path)
    assert not torch.equal(fresh._engine.params, eng.params) and bool(torch.isfinite(eng.params).all())
    assert torch.equal(eng.params, eng.params_tgt)
    # two runs from the same seeds: bit-identical parameters, simulator, replay arrays and loss logs
    t2, sim2, replay2, out2 = run(kind, tmp_path)
    assert_same(snapshot(t, sim, replay), snapshot(t2, sim2, replay2))
    assert (out["losses"] == out2["losses"]).all() and (out["tallies"] == out2["tallies"]).all()
    # a hand-written loop on sample_indices + dist_learn reproduces them bit for bit
    t3, sim3, replay3, losses3 = hand_written(kind, tmp_path)
    assert_same(snapshot(t, sim, replay), snapshot(t3, sim3, replay3))
    assert (out["losses"] == losses3).all()
    # the target equals the online network exactly where a sync is due (after blocks 0 and 2) and differs in between
    ta, *_ = run(kind, tmp_path, n_steps=BLOCK)
    assert torch.equal(ta._engine.params, ta._engine.params_tgt) and ta.epsilon == 0.5
    assert not torch.equal(ta._engine.params, fresh._engine.params)
    tb, *_ = run(kind, tmp_path, n_steps=2 * BLOCK)
    assert not torch.equal(tb._engine.params, tb._engine.params_tgt) and tb.epsilon == 0.25
    # a second call continues the first: 16 + 32 steps are the 48-step run
    sim_c, tc, replay_c = make_sim(), make_trainer(kind, tmp_path), DeviceReplay(2000, S, DEV)
    kw = dict(replay=replay_c, learning_starts=STARTS, block=BLOCK, seed=LOOP_SEED)
    first = tc.train_vectorized_dist(sim_c, BLOCK, **kw)
    second = tc.train_vectorized_dist(sim_c, 2 * BLOCK, **kw)
    assert_same(snapshot(t, sim, replay), snapshot(tc, sim_c, replay_c))
    assert first["learn_steps"] + second["learn_steps"] == STEPS - 1


def test_default_learning_starts_follow_train_online(tmp_path):
    """C51 starts at batch_size (32 <= 64 rows after one step), QR-DQN at training_learning_step (100: after two)."""
    c51 = make_trainer("c51", tmp_path)
    assert c51.train_vectorized_dist(make_sim(), 2)["learn_steps"] == 2
    qr = make_trainer("qr", tmp_path, transition_learning_step=100)
    assert qr.train_vectorized_dist(make_sim(), 2)["learn_steps"] == 1
    assert c51.device_replay.capacity == 100000 and len(qr.device_replay) == 128


def test_refusals(tmp_path):
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.train.c51_trainer import C51Trainer
    from porl_amd.train.dqn_trainer import DQNTrainer
    from porl_amd.train.qr_dqn_trainer import QRDQNTrainer
    from porl_amd.train.vector_online import train_vectorized_dist
    sim = make_sim()
    dqn = DQNTrainer(S, A, 0.99, device=DEV, batch_size=B, log_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="C51Trainer and QRDQNTrainer"):
        train_vectorized_dist(dqn, sim, 4)
    assert dqn.optimizer.step_count == 0 and not hasattr(dqn, "_vec_steps")

    class Acts(C51Trainer):
        def select_action(self, state):
            return 0

    class Learns(QRDQNTrainer):
        def learn_on(self, *batch):
            return super().learn_on(*batch)

    class LearnsWhole(QRDQNTrainer):
        def learn(self):
            return super().learn()

    for kind, cls in (("c51", Acts), ("qr", Learns), ("qr", LearnsWhole)):
        sub = make_trainer(kind, tmp_path, cls=cls)
        with pytest.raises(NotImplementedError, match=r"train_online\(Env\("):
            sub.train_vectorized_dist(sim, 4)
        assert sub.optimizer.step_count == 0 and not hasattr(sub, "_vec_steps")
    for kind in ("c51", "qr"):
        t = make_trainer(kind, tmp_path)
        with pytest.raises(ValueError, match="auto_reset"):
            t.train_vectorized_dist(make_sim(auto_reset=False), 4)
        with pytest.raises(ValueError, match="observes"):
            t.train_vectorized_dist(make_sim(n_beams=20), 4)
        with pytest.raises(ValueError, match="observes"):
            t.train_vectorized_dist(make_sim(n_actions=4), 4)
        with pytest.raises(ValueError, match="learning_starts"):
            t.train_vectorized_dist(sim, 4, replay=DeviceReplay(100, S, DEV), learning_starts=101)
        assert t.optimizer.step_count == 0 and not hasattr(t, "_vec_steps") and not hasattr(t, "device_replay")
