"""PERTrainer.train_online on its one-launch pieces (csrc/per_online.hpp): golden parity with the reference's own loop
(scripts/gen_golden_online_per.py on tests/helpers/online_env.py), PrioritizedReplayBuffer.record against add + flush,
sample_slots against sample, the fused priority write-back against porl_per_update, the fast path against the loop on
select_action / add / learn, the tree invariant after a run that wraps the ring, and the fallback for wide states."""
import contextlib
import io
import random

import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from helpers.online_env import RecordingLogger, ToyEnv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
KEYS = ("states", "actions", "rewards", "next_states", "dones")


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _refuse(*a, **k):
    raise AssertionError("train_online left its one-launch path")


def _np_sd(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


def _losses(logger):
    return [c[4] for c in logger.calls if c[0] == "log_step" and c[4] is not None]


# -- 1. golden parity -------------------------------------------------------------------------------------------------
def _golden_trainer(z, per_sample_weights=False):
    from porl_amd.train.dqn_per_trainer import PERTrainer
    S, A, EP, MS, B, TF, CAP, seed_model, seed_env, seed_np, seed_rand = (int(v) for v in z["meta"])
    eps, eps_min, decay, gamma = (float(v) for v in z["eps"])
    t = PERTrainer(S, A, gamma, eps, eps_min, decay, TF, DEV, batch_size=B, capacity=CAP, per_sample_weights=per_sample_weights)
    assert (t.memory.alpha, t.memory.beta_start) == (float(z["per"][0]), float(z["per"][1]))
    t.memory.beta_frames = int(z["per"][2])
    init = {k: torch.from_numpy(v) for k, v in sub(z, "init/").items()}
    t.q_network.load_state_dict(init)
    t.target_network.load_state_dict(init)
    t.logger = RecordingLogger()
    return t, EP, MS, seed_env, seed_np, seed_rand


def _refuse_host_paths(t, monkeypatch):
    from porl_amd import engine as E
    t.select_action = t.get_action = _refuse
    t.memory.sample = t.memory._flush = _refuse
    monkeypatch.setattr(E, "gather_rows", _refuse)


def test_per_train_online_matches_reference_golden(monkeypatch):
    z, _ = load_golden("online_per_s8_a4")
    assert float(z["min_gap"]) >= 1e-3 and float(z["min_margin"]) >= 5e-5 and int(z["n_resample"]) == 0
    t, EP, MS, seed_env, seed_np, seed_rand = _golden_trainer(z)
    _refuse_host_paths(t, monkeypatch)
    env = ToyEnv(seed=seed_env)
    np.random.seed(seed_np)
    random.seed(seed_rand)
    rewards = _quiet(t.train_online, env, num_episodes=EP, max_steps=MS)
    np.testing.assert_array_equal(np.array(env.actions), z["actions"])
    np.testing.assert_array_equal(np.array(rewards, dtype=np.float64), z["rewards_history"])
    assert t.epsilon == float(z["final_epsilon"])
    calls = [c for c in t.logger.calls if c[0] in ("log_step", "log_episode")]
    got = np.array([[0, c[1], c[2], c[4] is not None] if c[0] == "log_step" else [1, c[1], -1, 0] for c in calls])
    np.testing.assert_array_equal(got, z["log_calls"])
    assert t.logger.calls[-1] == ("close",) and env.closed
    mem = t.memory
    assert (mem.n_entries, mem.data_pointer, mem.frame_count) == (int(z["n_entries"]), int(z["data_pointer"]), int(z["frame_count"]))
    assert float(mem.beta) == float(z["beta"])
    assert mem._pending == []
    n = mem.n_entries
    for k in KEYS:
        np.testing.assert_array_equal(mem._store[k][:n].cpu().numpy().reshape(z["buf/" + k].shape), z["buf/" + k], err_msg=k)
    losses = _losses(t.logger)
    assert all(isinstance(v, float) for v in losses)
    print("loss max rel err", np.max(np.abs(np.array(losses) - z["losses"]) / np.abs(z["losses"])))
    tree = mem.tree.cpu().numpy()
    print("tree max abs err", np.max(np.abs(tree - z["tree"])), "max rel err on leaves",
          np.max(np.abs(tree - z["tree"])[z["tree"] > 0] / z["tree"][z["tree"] > 0]))
    np.testing.assert_allclose(losses, z["losses"], rtol=1e-4, atol=1e-7)
    for pre, mod in (("final/", t.q_network), ("final_target/", t.target_network)):
        want, have = sub(z, pre), _np_sd(mod)
        assert list(have) == list(want)
        for k in want:
            np.testing.assert_allclose(have[k], want[k], rtol=1e-4, atol=2e-6, err_msg=pre + k)
    np.testing.assert_allclose(tree, z["tree"], rtol=2e-5, atol=5e-6)


# -- 2. record == add + flush -----------------------------------------------------------------------------------------
def _transitions(n, S, seed):
    rng = np.random.default_rng(seed)
    return [(float(abs(rng.standard_normal()) + 0.01), rng.standard_normal(S).astype(np.float32), int(rng.integers(0, 6)),
             float(rng.standard_normal()), rng.standard_normal(S).astype(np.float32), bool(rng.random() < 0.2))
            for _ in range(n)]


def _assert_twins(a, b):
    b._flush()
    assert a._pending == [] and (a.data_pointer, a.n_entries) == (b.data_pointer, b.n_entries)
    assert torch.equal(a.tree, b.tree)
    for k in KEYS:
        assert torch.equal(a._store[k], b._store[k]), k
    assert int(a._stamp.abs().sum()) == 0 and int(b._stamp.abs().sum()) == 0


def test_record_wraps_and_matches_add_twin():
    from porl_amd.buffer.prioritized_replay_buffer import PrioritizedReplayBuffer
    S, cap, B = 6, 37, 8
    a, b = (PrioritizedReplayBuffer(cap, beta_frames=50, device=DEV) for _ in range(2))
    rng = np.random.default_rng(5)
    checks = 0
    for i, tr in enumerate(_transitions(3 * cap + 5, S, seed=1)):
        assert a.record(*tr) is True
        b.add(*tr)
        if i % 9 == 8:
            _assert_twins(a, b)
            random.seed(i)
            slots, w, wmean, idx = a.sample_slots(B)
            state_a = random.getstate()
            random.seed(i)
            *rows, w_b, idx_b = b.sample(B)
            assert random.getstate() == state_a
            assert torch.equal(idx, idx_b) and torch.equal(w, w_b) and torch.equal(rows[0], a._store["states"][slots])
            # priority write-back naming one leaf twice: the later value wins, in both forms
            idx = idx.clone()
            idx[5] = idx[3]
            td = torch.from_numpy(np.abs(rng.standard_normal(B)).astype(np.float32)).to(DEV)
            a.update_priorities_device(idx, td)
            b.update_priorities(idx, td)
            _assert_twins(a, b)
            checks += 1
    _assert_twins(a, b)
    assert checks >= 12 and (a.n_entries, a.data_pointer) == (cap, (3 * cap + 5) % cap)
    t = a.tree.cpu().numpy()
    inner = np.arange(cap - 1)
    assert np.array_equal(t[inner], t[2 * inner + 1] + t[2 * inner + 2])


def test_record_after_pending_adds_keeps_their_order():
    from porl_amd.buffer.prioritized_replay_buffer import PrioritizedReplayBuffer
    S, cap = 4, 5
    a, b = (PrioritizedReplayBuffer(cap, device=DEV) for _ in range(2))
    trs = _transitions(13, S, seed=2)
    for i, tr in enumerate(trs):
        b.add(*tr)
        if i % 3 == 2:
            assert a.record(*tr)                       # flushes the two queued adds first
            assert a._pending == []
        else:
            a.add(*tr)
    assert len(a._pending) == 1                        # the last transition was a plain add
    a._flush()
    _assert_twins(a, b)


# -- 3. sample_slots == sample ----------------------------------------------------------------------------------------
def _filled(z, how):
    from porl_amd.buffer.prioritized_replay_buffer import PrioritizedReplayBuffer
    cap, n, S, B, seed = (int(v) for v in z["meta"])
    buf = PrioritizedReplayBuffer(cap, alpha=0.6, beta_start=0.4, beta_frames=1000, device=DEV)
    for i in range(n):
        getattr(buf, how)(z["td"][i], z["st"][i], int(z["ac"][i]), float(z["rw"][i]), z["ns"][i], float(z["dn"][i]))
    return buf, cap, B, seed


def test_sample_slots_is_sample_without_the_gathers():
    from porl_amd import _native as N
    z, _ = load_golden("per_cap300")
    a, cap, B, seed = _filled(z, "record")
    b, *_ = _filled(z, "add")
    for k in range(3):
        random.seed(seed + k)
        u = [random.random() for _ in range(B)]
        random.seed(seed + k)
        slots, w, wmean, idx = a.sample_slots(B)
        state_a = random.getstate()
        random.seed(seed + k)
        *_, w_b, idx_b = b.sample(B)
        assert random.getstate() == state_a
        assert torch.equal(idx, idx_b) and torch.equal(w, w_b)
        assert slots.dtype == torch.int64 and torch.equal(slots, idx - (cap - 1))
        assert float(a.beta) == float(b.beta) and a.frame_count == b.frame_count == k + 1
        assert wmean.shape == (1,) and wmean.dtype == torch.float32
        # the mean as specified: the raw weights porl_per_sample leaves behind, summed in fp64 in index order, / max / B
        ud = torch.tensor(u, dtype=torch.float64, device=DEV)
        o_idx = torch.empty(B, dtype=torch.int64, device=DEV)
        o_prio = torch.empty(2 * B, dtype=torch.float64, device=DEV)
        o_w = torch.empty(B, dtype=torch.float32, device=DEV)
        N.check(N.lib().porl_per_sample(N.ptr(b.tree), cap, N.ptr(ud), B, b.n_entries, float(b.beta), N.ptr(o_idx), N.ptr(o_prio),
                                        N.ptr(o_w), N.current_stream_ptr(DEV)))
        assert torch.equal(o_idx, idx) and torch.equal(o_w, w)
        raw = o_prio[B:].cpu().numpy()
        total = 0.0
        for v in raw:
            total += float(v)
        assert np.float32(wmean.item()) == np.float32(total / raw.max() / B)
        # and it is the mean of the weights: each fp32 weight is within 2^-24 of raw / max, one more rounding at the end
        mean64 = float(np.mean(w.cpu().numpy().astype(np.float64)))
        assert abs(float(wmean.item()) - mean64) <= 2.0 ** -23 * mean64
        td = torch.rand(B, device=DEV) + 0.01
        a.update_priorities_device(idx, td)
        b.update_priorities(idx, td)
    assert torch.equal(a.tree, b.tree)


def test_sample_slots_on_the_reference_golden():
    z, _ = load_golden("per_cap300")
    buf, cap, B, seed = _filled(z, "record")
    assert len(buf) == cap and buf._pending == []
    random.seed(seed)
    for k in range(2):
        slots, w, wmean, idx = buf.sample_slots(B)
        assert np.array_equal(idx.cpu().numpy(), z[f"idx{k}"])
        np.testing.assert_allclose(w.cpu().numpy(), z[f"w{k}"], rtol=2e-7)
        assert np.array_equal(buf._store["states"][slots].cpu().numpy(), z[f"s{k}"])
        np.testing.assert_allclose(wmean.item(), z[f"w{k}"].mean(), rtol=3e-7)
    buf.update_priorities(list(z["upd_idx"]), z["upd_td"])          # contains one leaf twice: the later value wins
    slots, w, wmean, idx = buf.sample_slots(B)
    assert np.array_equal(idx.cpu().numpy(), z["idx2"])
    np.testing.assert_allclose(w.cpu().numpy(), z["w2"], rtol=2e-7)
    np.testing.assert_allclose(buf.tree.cpu().numpy(), z["tree_after"], rtol=1e-12, atol=1e-13)
    assert abs(float(buf.beta) - float(z["beta"])) < 1e-15


# -- 4. fused write-back == porl_per_update ----------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [300, 1000, 1])
@pytest.mark.parametrize("B", [1, 64, 1500])
def test_fused_write_back_is_porl_per_update(cap, B):
    from porl_amd.buffer.prioritized_replay_buffer import PrioritizedReplayBuffer
    a, b = (PrioritizedReplayBuffer(cap, device=DEV, state_shape=(2,)) for _ in range(2))
    rng = np.random.default_rng(1000 * cap + B)
    init_idx = torch.arange(cap, device=DEV) + (cap - 1)
    init_td = torch.from_numpy(rng.uniform(0.01, 2.0, size=cap)).to(DEV)
    for buf in (a, b):
        buf._update(init_idx, init_td)
    assert torch.equal(a.tree, b.tree)
    for rep in range(3):
        idx_np = rng.integers(cap - 1, 2 * cap - 1, size=B)
        if B > 5:
            idx_np[5] = idx_np[3]                                  # a leaf named twice, whatever else collides
        idx = torch.from_numpy(idx_np).to(DEV)
        td = torch.from_numpy(rng.uniform(-3.0, 3.0, size=B).astype(np.float32)).to(DEV)
        a.update_priorities_device(idx, td)
        b._update(idx, td.to(torch.float64))
        assert torch.equal(a.tree, b.tree)
        assert int(a._stamp.abs().sum()) == 0 and int(b._stamp.abs().sum()) == 0
    t = a.tree.cpu().numpy()
    inner = np.arange(cap - 1)
    assert np.array_equal(t[inner], t[2 * inner + 1] + t[2 * inner + 2])
    last = {int(i): float(v) for i, v in zip(idx_np, td.cpu().numpy())}          # the last writer of each leaf
    for i, v in last.items():
        np.testing.assert_allclose(t[i], (abs(v) + a.epsilon) ** a.alpha, rtol=1e-13)


# -- 5. fast path against the loop on select_action / add / learn ------------------------------------------------------
def _run_golden_config(z, fast, per_sample_weights, monkeypatch, episodes=None):
    from porl_amd.train import online
    t, EP, MS, seed_env, seed_np, seed_rand = _golden_trainer(z, per_sample_weights)
    with monkeypatch.context() as m:
        if fast:
            _refuse_host_paths(t, m)
        else:
            m.setattr(online, "fast_per_ok", lambda trainer: False)
        env = ToyEnv(seed=seed_env)
        np.random.seed(seed_np)
        random.seed(seed_rand)
        rewards = _quiet(t.train_online, env, num_episodes=episodes or EP, max_steps=MS)
    for k in ("sample", "_flush"):
        t.memory.__dict__.pop(k, None)
    return t, env, rewards


@pytest.mark.parametrize("per_sample_weights", [False, True])
def test_fast_path_equals_reference_loop(per_sample_weights, monkeypatch):
    z, _ = load_golden("online_per_s8_a4")
    a, env_a, ra = _run_golden_config(z, True, per_sample_weights, monkeypatch)
    b, env_b, rb = _run_golden_config(z, False, per_sample_weights, monkeypatch)
    assert env_a.actions == env_b.actions and ra == rb
    shape = lambda calls: [c[:3] + (c[4] is None,) if c[0] == "log_step" else c[:2] for c in calls]
    assert shape(a.logger.calls) == shape(b.logger.calls)
    la, lb = _losses(a.logger), _losses(b.logger)
    assert len(la) > 20
    np.testing.assert_allclose(la, lb, rtol=1e-5)
    for x, y in zip(a.q_network.parameters(), b.q_network.parameters()):
        np.testing.assert_allclose(x.detach().cpu().numpy(), y.detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    b.memory._flush()
    assert (a.memory.n_entries, a.memory.data_pointer, a.memory.frame_count) == \
           (b.memory.n_entries, b.memory.data_pointer, b.memory.frame_count)
    for k in KEYS:
        assert torch.equal(a.memory._store[k], b.memory._store[k]), k
    if not per_sample_weights:
        assert env_a.actions == list(z["actions"])
    else:                                                   # the weighting reaches the step: not the other setting's run
        assert len(la) != len(z["losses"]) or not np.allclose(la, z["losses"], rtol=1e-4, atol=1e-7)


def test_async_losses_reach_the_logger_as_device_statistics():
    z, _ = load_golden("online_per_s8_a4")
    t, EP, MS, seed_env, seed_np, seed_rand = _golden_trainer(z)
    t.async_losses = True
    t.select_action = _refuse
    np.random.seed(seed_np)
    random.seed(seed_rand)
    _quiet(t.train_online, ToyEnv(seed=seed_env), num_episodes=2, max_steps=MS)
    losses = _losses(t.logger)
    assert losses and all(isinstance(v, torch.Tensor) and v.device.type == "cuda" for v in losses)


# -- 6. tree invariant after a run that wraps the ring ------------------------------------------------------------------
def test_tree_invariant_after_a_wrapping_run(monkeypatch):
    z, _ = load_golden("online_per_s8_a4")
    t, env, _ = _run_golden_config(z, True, False, monkeypatch, episodes=12)
    mem = t.memory
    cap = mem.capacity
    assert len(env.actions) > cap and mem.n_entries == cap and mem.data_pointer == len(env.actions) % cap
    tree = mem.tree.cpu().numpy()
    inner = np.arange(cap - 1)
    assert np.array_equal(tree[inner], tree[2 * inner + 1] + tree[2 * inner + 2])
    assert (tree[cap - 1:] > 0).all() and tree[0] == mem.total_priority()
    assert int(mem._stamp.abs().sum()) == 0
    assert np.isfinite(_losses(t.logger)).all()


# -- 7. fallback: a state wider than the record kernel's arguments ------------------------------------------------------
class _Counter:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return 0.125 * self.n


@pytest.fixture
def track_episode_lengths(monkeypatch):
    orig_step, orig_reset = ToyEnv.step, ToyEnv.reset

    def reset(self, seed=None):
        self._ep_len = getattr(self, "_ep_len", [])
        self._ep_len.append(0)
        return orig_reset(self, seed)

    def step(self, action):
        self._ep_len[-1] += 1
        return orig_step(self, action)
    monkeypatch.setattr(ToyEnv, "reset", reset)
    monkeypatch.setattr(ToyEnv, "step", step)


def _check_semantics(t, env, threshold, episodes=4, max_steps=30):
    """The loop's call sequence (dqn_per_trainer.py:127-175): per step a reward-only log_step, then — once the memory
    holds `threshold` transitions — one policy() call and a log_step with its loss; per episode the epsilon decay, the
    target sync every update_target_freq episodes, log_episode; close() at the end."""
    log = t.logger = RecordingLogger()
    orig_sync = t.sync_target
    t.sync_target = lambda: (log.calls.append(("sync",)), orig_sync())
    pol = _Counter()
    eps0, decay, eps_min = t.epsilon, t.epsilon_decay, t.epsilon_min
    np.random.seed(9)
    rewards = _quiet(t.train_online, env, pol, num_episodes=episodes, max_steps=max_steps)
    assert env.closed and log.calls[-1] == ("close",)
    want, n, k, eps, j = [], 0, 0, eps0, 0
    assert len(env._ep_len) == episodes
    for ep, steps in enumerate(env._ep_len):
        for step in range(steps):
            n += 1
            r = log.calls[j][3]
            want.append(("log_step", ep, step, r, None, eps))
            j += 1
            if n >= threshold:
                k += 1
                want.append(("log_step", ep, step, r, 0.125 * k, eps))
                j += 1
        eps = max(eps_min, eps * decay)
        if ep % t.update_target_freq == 0:
            want.append(("sync",))
            j += 1
        want.append(("log_episode", ep))
        j += 1
    want.append(("close",))
    assert log.calls == want
    assert pol.n == k == max(0, n - threshold + 1) > 0
    assert len(rewards) == episodes and t.epsilon == eps


def test_wide_state_falls_back_to_add_and_the_plain_loop(track_episode_lengths):
    from porl_amd.buffer.prioritized_replay_buffer import PrioritizedReplayBuffer
    from porl_amd.train import online
    from porl_amd.train.dqn_per_trainer import PERTrainer
    from porl_amd.train.cql_trainer import QnetEngine
    S = QnetEngine.RECORD_MAX_STATE + 1
    a, b = (PrioritizedReplayBuffer(5, device=DEV) for _ in range(2))
    for tr in _transitions(7, S, seed=3):
        assert a.record(*tr) is False                           # too wide for the arguments: add's deferred path
        b.add(*tr)
    assert len(a._pending) == 7
    a._flush()
    _assert_twins(a, b)
    ok = PrioritizedReplayBuffer(5, device=DEV)
    assert ok.record(*_transitions(1, S - 1, seed=4)[0]) is True  # the widest state that still rides in the arguments
    np.testing.assert_array_equal(ok._store["states"][0].cpu().numpy(), _transitions(1, S - 1, seed=4)[0][1])

    t = PERTrainer(S, 4, 0.99, epsilon=1.0, epsilon_decay=0.5, update_target_freq=2, device=DEV, batch_size=24, capacity=256)
    assert not online.fast_per_ok(t)
    acted = []
    orig = t.select_action
    t.select_action = lambda s: (acted.append(1), orig(s))[1]
    env = ToyEnv(seed=9, state_size=S)
    _check_semantics(t, env, threshold=24)
    assert len(acted) == len(env.actions) == sum(env._ep_len)    # every action came from select_action: the plain loop
    assert len(t.memory) == len(env.actions) and len(t.replay_buffer) == 0


def test_fast_path_keeps_the_loop_semantics(track_episode_lengths):
    from porl_amd.train import online
    from porl_amd.train.dqn_per_trainer import PERTrainer
    t = PERTrainer(8, 4, 0.99, epsilon=1.0, epsilon_decay=0.5, update_target_freq=2, device=DEV, batch_size=24)
    assert online.fast_per_ok(t)
    t.select_action = _refuse
    _check_semantics(t, ToyEnv(seed=9), threshold=24)
    assert len(t.memory) > 24 and t.memory._pending == [] and len(t.replay_buffer) == 0


def test_overridden_learn_or_action_rule_takes_the_plain_loop():
    from porl_amd.train.dqn_per_trainer import PERTrainer
    seen = []

    class MyLearn(PERTrainer):
        def learn(self):
            seen.append("learn")
            return super().learn()

    class MyAct(PERTrainer):
        def select_action(self, state):
            seen.append("act")
            return 1
    for cls, tag in ((MyLearn, "learn"), (MyAct, "act")):
        del seen[:]
        t = cls(8, 4, 0.99, epsilon=0.3, epsilon_decay=0.5, device=DEV, batch_size=8, capacity=128)
        t.logger = RecordingLogger()
        np.random.seed(0)
        random.seed(0)
        _quiet(t.train_online, ToyEnv(seed=2), num_episodes=3, max_steps=20)
        assert tag in seen
