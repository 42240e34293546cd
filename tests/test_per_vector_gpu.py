"""Prioritized replay for the vectorised loop (csrc/per_vector.hpp, porl_amd/train/vector_per.py): the range fill against
porl_per_update, the keyed sampler against porl_per_sample_slots fed the same uniforms, PrioritizedReplayBuffer as the replay
target of DiscreteLidarNavSim.step, and `train_vectorized_per` against a loop written out from calls that predate it.

Everything asserted is an identity (bit-equal trees, indices, weights, reruns, hand-written loop, counts) or finiteness: no
tolerance."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from helpers import per_vector_cases as PV
from porl_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _buffer(cap, **kw):
    from porl_amd.buffer.prioritized_replay_buffer import PrioritizedReplayBuffer
    return PrioritizedReplayBuffer(cap, device=DEV, state_shape=(2,), **kw)


def _leaf_value(td, eps=1e-5, alpha=0.6):
    """(|td| + eps)^alpha as the device computes it: one leaf set by porl_per_update."""
    b = _buffer(1, epsilon=eps, alpha=alpha)
    b._update(torch.zeros(1, dtype=torch.int64, device=DEV), torch.tensor([td], dtype=torch.float64, device=DEV))
    return float(b.tree[0])


def _boundary_slot(cap):
    """The data slot whose leaf is the first of the deepest level, 2^D - 1 (capacity not a power of two)."""
    D = (2 * cap - 1).bit_length() - 1
    return (1 << D) - 1 - (cap - 1)


# -- 1. the fill against porl_per_update ----------------------------------------------------------------------------------
FILLS = [
    (1, 0, 1), (2, 0, 1), (2, 1, 2), (3, 0, 3), (3, 2, 2), (3, 1, 1),          # the leaf is the root; the smallest trees
    (1000, 0, 1), (1000, 999, 1), (1000, 0, 1000), (1000, 377, 1000),            # two leaf depths; n = 1; n = capacity (wrapped too)
    (1000, 990, 64),                                                             # a wrapped range
    (1000, _boundary_slot(1000) - 5, 64), (1000, _boundary_slot(1000), 1), (1000, _boundary_slot(1000) - 1, 2),
    (1024, 0, 64), (1024, 1000, 64), (1024, 0, 1024), (1024, 513, 1),
    (5000, 0, 64), (5000, 4990, 1024), (5000, 1000, 3000),                       # n = 3000: more than one pass of 1024 lanes,
    (5000, _boundary_slot(5000) - 1500, 3000), (5000, 0, 5000),                  # across the level boundary too
]


@pytest.mark.parametrize("cap,first,n", FILLS)
def test_fill_range_is_porl_per_update(cap, first, n):
    a, b = _buffer(cap), _buffer(cap)
    rng = np.random.default_rng(100003 * cap + 1009 * first + n)
    init_idx = torch.arange(cap, device=DEV) + (cap - 1)
    init_td = torch.from_numpy(rng.uniform(0.01, 2.0, size=cap)).to(DEV)
    for buf in (a, b):
        buf._update(init_idx, init_td)
    before = a.tree.cpu().numpy().copy()
    assert torch.equal(a.tree, b.tree) and np.array_equal(before, PV.rebuild(before, cap))
    td = float(rng.uniform(-3.0, 3.0))
    slots = (first + torch.arange(n, device=DEV)) % cap
    assert 1 <= n <= cap
    a.fill_range(first, n, td)
    b._update(slots + (cap - 1), torch.full((n,), td, dtype=torch.float64, device=DEV))
    assert torch.equal(a.tree, b.tree)
    t = a.tree.cpu().numpy()
    assert np.array_equal(t, PV.rebuild(t, cap))
    leaf = _leaf_value(td)
    assert (t[slots.cpu().numpy() + cap - 1] == leaf).all()
    outside = np.ones(2 * cap - 1, bool)
    outside[sorted(PV.range_nodes(cap, first, n))] = False
    assert np.array_equal(t[outside], before[outside])
    assert (a.data_pointer, a.n_entries) == (0, 0)               # fill_range moves no pointer


def test_level_boundary_cases_cross_the_boundary():
    for cap in (1000, 5000):
        s = _boundary_slot(cap)
        D = (2 * cap - 1).bit_length() - 1
        assert 0 < s < cap and s + cap - 1 == 2 ** D - 1
    assert any(f < _boundary_slot(c) < f + n <= c for c, f, n in FILLS if c == 1000)
    assert any(f < _boundary_slot(c) < f + n <= c and n > 1024 for c, f, n in FILLS if c == 5000)


@pytest.mark.parametrize("cap", [1000, 5000])
def test_two_fills_back_to_back(cap):
    a, b = _buffer(cap), _buffer(cap)
    rng = np.random.default_rng(cap)
    init_idx = torch.arange(cap, device=DEV) + (cap - 1)
    init_td = torch.from_numpy(rng.uniform(0.01, 2.0, size=cap)).to(DEV)
    for buf in (a, b):
        buf._update(init_idx, init_td)
    fills = [(cap - 300, 700, 0.7), (200, 640, -1.9)]                                  # the second overlaps the first's head
    for first, n, td in fills:                                                       # no synchronisation in between
        a.fill_range(first, n, td)
    for first, n, td in fills:
        slots = (first + torch.arange(n, device=DEV)) % cap
        b._update(slots + (cap - 1), torch.full((n,), td, dtype=torch.float64, device=DEV))
    assert torch.equal(a.tree, b.tree)
    t = a.tree.cpu().numpy()
    assert np.array_equal(t, PV.rebuild(t, cap))


# -- 2. the keyed sampler against porl_per_sample_slots ----------------------------------------------------------------------
def _tree(cap, n_entries):
    buf = _buffer(cap)
    rng = np.random.default_rng(7 * cap + n_entries)
    td = 10.0 ** rng.uniform(-2.0, 2.0, size=n_entries)                               # four decades
    buf._update(torch.arange(n_entries, device=DEV) + (cap - 1), torch.from_numpy(td).to(DEV))
    return buf


def _sample(buf, n_entries, B, u=None, seed=0, draw=0, beta=0.4):
    idx = torch.full((2, B), -1, dtype=torch.int64, device=DEV)
    w = torch.full((B + 1,), -1.0, dtype=torch.float32, device=DEV)
    raw = torch.zeros(B, dtype=torch.float64, device=DEV)
    tail = (N.ptr(idx[0]), N.ptr(idx[1]), N.ptr(w), C.c_void_p(w.data_ptr() + 4 * B), N.ptr(raw), N.current_stream_ptr(buf.device))
    if u is None:
        N.check(N.lib().porl_per_sample_keyed(N.ptr(buf.tree), buf.capacity, seed, draw, B, n_entries, beta, *tail), "keyed")
    else:
        N.check(N.lib().porl_per_sample_slots(N.ptr(buf.tree), buf.capacity, N.ptr(u), B, n_entries, beta, *tail), "slots")
    return idx[0], idx[1], w[:B], w[B:]


@pytest.mark.parametrize("B", [1, 32, 300])
@pytest.mark.parametrize("cap,n_entries", [(1000, 700), (1000, 1000), (1024, 333), (1024, 1024)])
def test_sample_keyed_is_sample_slots_on_keyed_u(cap, n_entries, B):
    buf = _tree(cap, n_entries)
    seed = 2 ** 63 + 12345
    outs = {}
    for draw in (0, 1, 2 ** 32 - 1):
        got = _sample(buf, n_entries, B, seed=seed, draw=draw)
        u = torch.from_numpy(PV.keyed_us(seed, draw, B)).to(DEV)
        want = _sample(buf, n_entries, B, u=u)
        for g, x in zip(got, want):
            assert torch.equal(g, x)
        tree_idx, slots, w, wmean = got
        assert torch.equal(slots, tree_idx - (cap - 1)) and int(slots.min()) >= 0 and int(slots.max()) < n_entries
        assert bool(torch.isfinite(w).all()) and float(w.max()) == 1.0 and 0.0 < float(wmean) <= 1.0
        again = _sample(buf, n_entries, B, seed=seed, draw=draw)                     # the same draw repeats
        for g, x in zip(got, again):
            assert torch.equal(g, x)
        outs[draw] = got
    if B > 1:                                                                        # two different draws differ
        assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[1][0], outs[2 ** 32 - 1][0])
    else:
        firsts = {int(_sample(buf, n_entries, 1, seed=seed, draw=d)[0]) for d in range(8)}
        assert len(firsts) > 1
    other = _sample(buf, n_entries, B, seed=seed + 1, draw=0)                        # and so do two seeds
    assert B == 1 or not torch.equal(other[0], outs[0][0])


# -- 3. the buffer as a replay target -----------------------------------------------------------------------------------------
N_ENVS, N_BEAMS, S, A, B, STEPS, BLOCK, STARTS, SEED, CAP = 64, 36, 38, 5, 32, 48, 16, 128, 5, 2000


def make_sim():
    from porl_amd.env import DiscreteLidarNavSim, NavWorld
    return DiscreteLidarNavSim(NavWorld.lattice(), N_ENVS, n_actions=A, seed=3, auto_reset=True, n_beams=N_BEAMS, episode_step=20)


def test_buffer_is_a_replay_target():
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.buffer.prioritized_replay_buffer import PrioritizedReplayBuffer
    mem, plain = PrioritizedReplayBuffer(CAP, state_shape=(S,), device=DEV), DeviceReplay(CAP, S, DEV)
    assert mem.state_dim == S and mem.position == 0 and mem.priority_for_new == 1.0 and mem.states.shape == (CAP, S)
    sim_a, sim_b = make_sim(), make_sim()
    sim_a.reset(), sim_b.reset()
    g = torch.Generator().manual_seed(1)
    leaf = _leaf_value(1.0)
    for step in range(1, 36):                                       # 35 * 64 = 2240 rows: the ring wraps
        acts = torch.randint(0, A, (N_ENVS,), generator=g).to(DEV)
        sim_a.step(acts, replay=mem)
        sim_b.step(acts, replay=plain)
        if step in (1, 17, 31, 32, 35):
            rows = min(N_ENVS * step, CAP)
            assert len(mem) == len(plain) == rows and mem.data_pointer == mem.position == plain.position == N_ENVS * step % CAP
            want = np.zeros(2 * CAP - 1)
            want[CAP - 1:CAP - 1 + rows] = leaf
            assert np.array_equal(mem.tree.cpu().numpy(), PV.rebuild(want, CAP))
    for x, y in zip(mem.arrays(), plain.arrays()):
        assert torch.equal(x, y)
    assert torch.equal(sim_a.state, sim_b.state) and torch.equal(sim_a.obs, sim_b.obs)
    # the keyed sampler takes nothing from Python's generator, and keeps sample_slots' bookkeeping
    random.seed(11)
    state = random.getstate()
    frames = mem.frame_count
    slots, w, wmean, tree_idx = mem.sample_slots_keyed(B, SEED, 0)
    assert random.getstate() == state and mem.frame_count == frames + 1 and mem.beta == mem.beta_start
    assert slots.shape == w.shape == tree_idx.shape == (B,) and wmean.shape == (1,)
    assert torch.equal(slots, tree_idx - (CAP - 1)) and int(slots.max()) < CAP
    # a host add still works on the same memory: it lands in the slot the ring points at
    p = mem.data_pointer
    mem.add(2.0, np.ones(S, np.float32), 1, 0.5, np.zeros(S, np.float32), False)
    mem.priority_for_new = 0.25
    sim_a.step(acts, replay=mem)                                     # flushes the pending add before the device write
    t = mem.tree.cpu().numpy()
    assert mem._pending == [] and t[CAP - 1 + p] == _leaf_value(2.0) and t[CAP - 1 + p + 1] == _leaf_value(0.25)
    assert np.array_equal(t, PV.rebuild(t, CAP)) and bool((mem.states[p] == 1.0).all())


# -- 4. the loop --------------------------------------------------------------------------------------------------------------
KINDS = {"mean_weight": (False, [64, 64]), "per_sample": (True, [64, 64]), "wide": (False, [256, 256])}


def make_trainer(kind, tmp_path):
    from porl_amd.net.q_network import QNetwork
    from porl_amd.train.dqn_per_trainer import PERTrainer
    psw, hidden = KINDS[kind]
    torch.manual_seed(0)
    return PERTrainer(S, A, 0.99, epsilon=1.0, epsilon_min=0.05, epsilon_decay=0.5, update_target_freq=2, device=DEV, batch_size=B,
                      log_dir=str(tmp_path), capacity=CAP, per_sample_weights=psw, network=lambda s, a: QNetwork(s, a, hidden))


def run(kind, tmp_path, n_steps=STEPS):
    t, sim = make_trainer(kind, tmp_path), make_sim()
    out = t.train_vectorized_per(sim, n_steps, learn_per_step=1, learning_starts=STARTS, block=BLOCK, seed=SEED)
    return t, sim, out


def snapshot(t, sim):
    eng, mem = t._engine, t.memory
    xs = [eng.params, eng.params_tgt, eng.adam_m, eng.adam_v, sim.state, sim.counters, sim.obs, sim.tallies, mem.tree,
          *(mem._store[k] for k in ("states", "actions", "rewards", "next_states", "dones")),
          torch.tensor([mem.data_pointer, mem.n_entries, mem.frame_count, t.optimizer.step_count])]
    return [x.clone() for x in xs]


def assert_same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), k


def hand_written(kind, tmp_path):
    """The loop from calls that predate it: sim.step into a plain DeviceReplay, the rows copied into the memory's store,
    memory._update over the range, porl_per_sample_slots fed keyed_u, learn_indexed, update_priorities_device."""
    from porl_amd.buffer.device_replay import DeviceReplay
    t, sim = make_trainer(kind, tmp_path), make_sim()
    eng, mem = t._engine, t.memory
    plain = DeviceReplay(CAP, S, DEV)
    st = mem._store
    views = (st["states"], st["actions"], st["rewards"].view(-1), st["next_states"], st["dones"].view(-1))
    sim.reset()
    q = torch.empty(N_ENVS, A, device=DEV)
    acts = torch.empty(N_ENVS, dtype=torch.int64, device=DEV)
    td_abs = t._td_abs[:B]
    losses, draw, eps = [], 0, 1.0
    for it in range(STEPS):
        eng.act_rows(sim.obs, eps, SEED, it, env_offset=0, q=q, out=acts)
        slots = (plain.position + torch.arange(N_ENVS, device=DEV)) % CAP
        sim.step(acts, replay=plain)
        for dst, src in zip(views, plain.arrays()):
            dst[slots] = src[slots]
        mem._update(slots + (CAP - 1), torch.full((N_ENVS,), t.max_initial_priority, dtype=torch.float64, device=DEV))
        mem.data_pointer, mem.n_entries = plain.position, len(plain)
        if len(plain) >= STARTS:
            beta = np.min([1.0, mem.beta_start + mem.frame_count * (1.0 - mem.beta_start) / mem.beta_frames])
            mem.beta, mem.frame_count = beta, mem.frame_count + 1
            u = torch.from_numpy(PV.keyed_us(SEED, draw, B)).to(DEV)
            tree_idx, rows, w, wmean = _sample(mem, mem.n_entries, B, u=u, beta=float(beta))
            hp = t.optimizer.hyper(t.gamma, 0.0, 1.0 / B)
            if t.per_sample_weights:
                var = N.QnetVariant(1, w.data_ptr(), None, td_abs.data_ptr())
            else:
                var = N.QnetVariant(1, None, wmean.data_ptr(), td_abs.data_ptr())
            eng.learn_indexed(hp, *views, rows, variant=var)
            t.optimizer.step_count = hp.step
            mem.update_priorities_device(tree_idx, td_abs)
            draw += 1
            losses.append(eng.stats[:1].clone())
        if (it + 1) % BLOCK == 0:
            eps = max(0.05, eps * 0.5)
            if ((it + 1) // BLOCK - 1) % 2 == 0:
                t.sync_target()
    return t, sim, torch.cat(losses).cpu().numpy()


@pytest.mark.parametrize("kind", list(KINDS))
def test_vectorized_per_training(kind, tmp_path):
    t, sim, out = run(kind, tmp_path)
    eng, mem = t._engine, t.memory
    assert eng.fused == (kind != "wide")                        # [256, 256] takes the multi-launch path
    assert out["transitions"] == N_ENVS * STEPS == 3072
    assert out["learn_steps"] == STEPS - 1 == t.optimizer.step_count == len(out["losses"]) == mem.frame_count        # (c)
    assert bool(np.isfinite(out["losses"]).all()) and (out["losses"] > 0).any()                                     # (d)
    assert len(mem) == CAP and mem.data_pointer == 3072 % CAP and t.epsilon == 0.125 and t._vec_steps == STEPS and t._draws == STEPS - 1
    tree = mem.tree.cpu().numpy()
    assert np.array_equal(tree, PV.rebuild(tree, CAP)) and out["total_priority"] == tree[0]                         # (e)
    assert bool((tree[CAP - 1:] != _leaf_value(t.max_initial_priority)).any()) and bool((tree[CAP - 1:] > 0).all())  # (f)
    assert (out["tallies"] == sim.tallies.sum(0).cpu().numpy()).all() and out["tallies"][0] >= 2 * N_ENVS
    assert not torch.equal(make_trainer(kind, tmp_path)._engine.params, eng.params)
    # (a) a rerun is bit-identical
    t2, sim2, out2 = run(kind, tmp_path)
    assert_same(snapshot(t, sim), snapshot(t2, sim2))
    assert (out["losses"] == out2["losses"]).all() and (out["tallies"] == out2["tallies"]).all()
    # (b) and so is the loop written out from the calls that predate it
    t3, sim3, losses3 = hand_written(kind, tmp_path)
    assert_same(snapshot(t, sim), snapshot(t3, sim3))
    assert (out["losses"] == losses3).all()


def test_a_second_call_continues_the_first(tmp_path):
    t, sim, out = run("mean_weight", tmp_path)
    tc, sim_c = make_trainer("mean_weight", tmp_path), make_sim()
    kw = dict(learning_starts=STARTS, block=BLOCK, seed=SEED)
    first = tc.train_vectorized_per(sim_c, BLOCK, **kw)
    assert (tc._vec_steps, tc._draws) == (BLOCK, BLOCK - 1)
    second = tc.train_vectorized_per(sim_c, 2 * BLOCK, **kw)                                                        # (g)
    assert_same(snapshot(t, sim), snapshot(tc, sim_c))
    assert first["learn_steps"] + second["learn_steps"] == STEPS - 1
    assert (np.concatenate([first["losses"], second["losses"]]) == out["losses"]).all()
    # a later learn() goes on from the same memory
    loss = tc.learn()
    assert np.isfinite(float(loss)) and tc.optimizer.step_count == STEPS
    with pytest.raises(NotImplementedError, match=r"train_online\(Env\("):                                         # (h)
        tc.train_vectorized(sim_c, 4)


def test_refusals_advance_nothing(tmp_path):
    from porl_amd.env import DiscreteLidarNavSim, NavWorld
    from porl_amd.train.dqn_trainer import DQNTrainer
    from porl_amd.train.dqn_per_trainer import PERTrainer
    from porl_amd.train.vector_online import train_vectorized_per
    t, sim = make_trainer("mean_weight", tmp_path), make_sim()
    with pytest.raises(ValueError, match="auto_reset"):
        t.train_vectorized_per(DiscreteLidarNavSim(NavWorld.lattice(), 8, n_beams=N_BEAMS), 4)
    with pytest.raises(ValueError, match="observes"):
        t.train_vectorized_per(DiscreteLidarNavSim(NavWorld.lattice(), 8, n_beams=20, auto_reset=True), 4)
    with pytest.raises(ValueError, match="learning_starts"):
        t.train_vectorized_per(sim, 4, learning_starts=CAP + 1)
    with pytest.raises(ValueError, match="positive"):
        t.train_vectorized_per(sim, 0)
    small = PERTrainer(S, A, 0.99, device=DEV, batch_size=B, log_dir=str(tmp_path), capacity=48)
    with pytest.raises(ValueError, match="robots > memory capacity"):
        small.train_vectorized_per(sim, 4, learning_starts=B)
    with pytest.raises(NotImplementedError, match="PERTrainer"):
        train_vectorized_per(DQNTrainer(S, A, 0.99, device=DEV, batch_size=B, log_dir=str(tmp_path)), sim, 4)
    for x in (t, small):
        assert x.optimizer.step_count == 0 and not hasattr(x, "_vec_steps") and not hasattr(x, "_draws")
        assert len(x.memory) == 0 and x.memory.data_pointer == 0 and x.memory.frame_count == 0 and float(x.memory.tree[0]) == 0.0
