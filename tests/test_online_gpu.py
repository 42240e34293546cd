"""train_online of the Q-learning trainers and its one-launch pieces (csrc/online.hpp): golden parity with the reference's
own loop (scripts/gen_golden_online.py on tests/helpers/online_env.py), porl_qnet_act against forward + argmax,
ReplayBuffer.record against push + _sync_mirror, and the loop's semantics for the trainers off the fast path."""
import contextlib
import io

import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from helpers.online_env import RecordingLogger, ToyEnv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _np_sd(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _refuse(*a, **k):
    raise AssertionError("train_online left its one-launch path")


# -- golden parity ----------------------------------------------------------------------------------------------------
def _golden_trainer(kind, z):
    from porl_amd.buffer.replay_buffer import ReplayBuffer
    from porl_amd.train.c51_trainer import C51Trainer
    from porl_amd.train.dqn_trainer import DDQNTrainer, DQNTrainer
    S, A, EP, MS, THR, B, TF, CAP, seed_env, seed_np, atoms = (int(v) for v in z["meta"])
    eps, eps_min, decay, gamma, v_min, v_max = (float(v) for v in z["eps"])
    rb = ReplayBuffer(CAP, (S,), DEV)
    if kind == "c51":
        t = C51Trainer(S, A, gamma, eps, eps_min, decay, TF, DEV, atom_size=atoms, v_min=v_min, v_max=v_max,
                       network_hidden_sizes=[int(h) for h in z["hidden"]], batch_size=B, replay_buffer=rb)
    else:
        cls = DQNTrainer if kind == "dqn" else DDQNTrainer
        t = cls(S, A, gamma, eps, eps_min, decay, TF, DEV, batch_size=B, replay_buffer=rb, transition_learning_step=THR)
    init = {k: torch.from_numpy(v) for k, v in sub(z, "init/").items()}
    t.q_network.load_state_dict(init)
    t.target_network.load_state_dict(init)
    t.logger = RecordingLogger()
    t.select_action = _refuse
    t.get_action = _refuse
    return t, EP, MS, seed_env, seed_np


@pytest.mark.parametrize("kind", ["dqn", "ddqn", "c51"])
def test_train_online_matches_reference_golden(kind):
    z, _ = load_golden(f"online_{kind}_s8_a4")
    assert float(z["min_gap"]) > 1e-3                    # greedy choices were never near a tie: exact actions are meaningful
    assert int(z["n_greedy"]) > 10 and len(z["losses"]) > 10
    t, EP, MS, seed_env, seed_np = _golden_trainer(kind, z)
    env = ToyEnv(seed=seed_env)
    np.random.seed(seed_np)
    rewards = _quiet(t.train_online, env, num_episodes=EP, max_steps=MS)
    np.testing.assert_array_equal(np.array(env.actions), z["actions"])
    np.testing.assert_array_equal(np.array(rewards, dtype=np.float64), z["rewards_history"])
    assert t.epsilon == float(z["final_epsilon"])
    calls = [c for c in t.logger.calls if c[0] in ("log_step", "log_episode")]
    got = np.array([[0, c[1], c[2], c[4] is not None] if c[0] == "log_step" else [1, c[1], -1, 0] for c in calls])
    np.testing.assert_array_equal(got, z["log_calls"])
    assert t.logger.calls[-1] == ("close",) and env.closed
    losses = [c[4] for c in calls if c[0] == "log_step" and c[4] is not None]
    assert all(isinstance(v, float) for v in losses)
    np.testing.assert_allclose(losses, z["losses"], rtol=1e-4, atol=1e-7)
    for pre, mod in (("final/", t.q_network), ("final_target/", t.target_network)):
        want, have = sub(z, pre), _np_sd(mod)
        assert list(have) == list(want)
        for k in want:
            np.testing.assert_allclose(have[k], want[k], rtol=1e-4, atol=2e-6, err_msg=pre + k)
    rb = t.replay_buffer
    n = rb.size
    assert rb.position == int(z["buf/position"])
    for k in ("states", "actions", "rewards", "next_states", "dones"):
        np.testing.assert_array_equal(getattr(rb, k)[:n], z["buf/" + k], err_msg=k)
        np.testing.assert_array_equal(rb._mirror[k][:n].cpu().numpy().reshape(getattr(rb, k)[:n].shape), z["buf/" + k],
                                      err_msg="mirror " + k)


# -- porl_qnet_act ----------------------------------------------------------------------------------------------------
def _engine(S, A, hidden, seed=0):
    from porl_amd.train.cql_trainer import QnetEngine
    eng = QnetEngine(S, A, hidden, 16, DEV)
    eng._ensure_bound()
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for v in eng.views(eng.params):
            fan_in = v.shape[-1] if v.dim() == 2 else 16
            v.copy_((torch.randn(v.shape, generator=g) / fan_in ** 0.5).to(DEV))
    return eng


def _rec():
    return torch.full((16,), -1, dtype=torch.int32).pin_memory()


def _act_all_ways(eng, q_fn, S, kw, seed=1):
    """porl_qnet_act on B = 1 and B = 8, inline and from rows of a device array, against argmax of q_fn(x)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rows = (1.5 * torch.randn(12, S, generator=g)).to(DEV)
    q = q_fn(rows).float().cpu()
    top = torch.sort(q, dim=1, descending=True).values
    clear = ((top[:, 0] - top[:, 1]) > 1e-5).numpy()           # rows whose argmax no summation order can flip
    assert clear.sum() >= 10
    want = q.argmax(dim=1).numpy()
    for B in (1, 8):
        for r0 in (0, 3):
            m = clear[r0:r0 + B]
            rec = _rec()
            eng.act(rec, states=rows, row=r0, batch=B, **kw)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(rec[:B].numpy()[m], want[r0:r0 + B][m])
            if B * S <= eng.ACT_MAX_INLINE:
                rec = _rec()
                eng.act(rec, inline=rows[r0:r0 + B].cpu().numpy(), batch=B, **kw)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(rec[:B].numpy()[m], want[r0:r0 + B][m])


@pytest.mark.parametrize("hidden", [[64, 128, 64], [256, 256], [48, 40]])
def test_act_matches_forward_argmax(hidden):
    S, A = 8, 4 if hidden != [48, 40] else 7
    eng = _engine(S, A, hidden, seed=len(hidden))
    assert eng.act_ok
    _act_all_ways(eng, lambda x: eng.forward(x), S, {})
    # the target parameters (which=1) are a separate image
    with torch.no_grad():
        eng.params_tgt.copy_(eng.params)
        eng.views(eng.params_tgt)[-1].add_(torch.tensor([0.0, 0.0, 50.0] + [0.0] * (A - 3), device=DEV))
    rec = _rec()
    eng.act(rec, inline=np.zeros(S, np.float32), which=1)
    torch.cuda.synchronize()
    assert int(rec[0]) == 2


def test_act_dueling_c51_qr():
    from porl_amd.train.c51_trainer import C51Trainer
    from porl_amd.train.dddqn_trainer import DDDQNTrainer
    from porl_amd.train.qr_dqn_trainer import QRDQNTrainer
    S, A = 8, 4
    torch.manual_seed(3)
    t = DDDQNTrainer(S, A, 0.99, device=DEV)
    _act_all_ways(t._engine, lambda x: t.q_network(x), S, {})
    c = C51Trainer(S, A, 0.99, device=DEV, atom_size=21, v_min=-3, v_max=3, network_hidden_sizes=[48, 40])
    kind, n_sub, support = c._act_epilogue()
    with torch.no_grad():
        for p in c.q_network.parameters():
            p.mul_(4.0)                                    # spread the expectations apart
    _act_all_ways(c._engine, lambda x: c.q_network.get_q_values(x), S, dict(kind=kind, n_act=A, n_sub=n_sub, support=support))
    qr = QRDQNTrainer(S, A, 0.99, device=DEV, num_quantiles=12, network_hidden_sizes=[64, 64])
    kind, n_sub, support = qr._act_epilogue()
    _act_all_ways(qr._engine, lambda x: qr.q_network.get_mean_q_values(x), S, dict(kind=kind, n_act=A, n_sub=n_sub))


def test_act_exact_tie_takes_lowest_index_and_copies_statistics():
    S, A = 8, 5
    eng = _engine(S, A, [64, 128, 64])
    with torch.no_grad():
        eng.views(eng.params)[-2].zero_()
        eng.views(eng.params)[-1].fill_(0.25)                        # every Q value 0.25 exactly
        eng.stats[:3].copy_(torch.tensor([1.5, -2.0, 3.25], device=DEV))
    rec = _rec()
    eng.act(rec, inline=np.ones(S, np.float32), n_stats=3)
    torch.cuda.synchronize()
    assert int(rec[0]) == 0
    np.testing.assert_array_equal(rec.view(torch.float32)[8:11].numpy(), np.array([1.5, -2.0, 3.25], np.float32))
    with torch.no_grad():
        eng.views(eng.params)[-1].copy_(torch.tensor([0.0, 1.0, 0.5, 1.0, -1.0], device=DEV))   # tie of actions 1 and 3
    x = torch.randn(8, S, device=DEV)
    rec = _rec()
    eng.act(rec, states=x, batch=8)
    torch.cuda.synchronize()
    assert rec[:8].tolist() == [1] * 8
    assert eng.forward(x).argmax(dim=1).tolist() == [1] * 8


@pytest.mark.parametrize("hidden", [[1024, 1024], [2048]])
def test_act_rejects_oversize_engine(hidden):
    from porl_amd.train.cql_trainer import QnetEngine
    eng = QnetEngine(8, 4, hidden, 8, DEV)
    eng._ensure_bound()
    assert not eng.act_ok
    with pytest.raises(RuntimeError, match="too large"):
        eng.act(_rec(), inline=np.zeros(8, np.float32))


# -- ReplayBuffer.record ----------------------------------------------------------------------------------------------
def _transitions(n, S, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(S).astype(np.float32), int(rng.integers(0, 6)), float(rng.standard_normal()),
             rng.standard_normal(S).astype(np.float32), bool(rng.random() < 0.2)) for _ in range(n)]


def _assert_mirror_is_host(rb):
    for k in ("states", "actions", "rewards", "next_states", "dones"):
        host = getattr(rb, k)
        np.testing.assert_array_equal(rb._mirror[k].cpu().numpy().reshape(host.shape), host, err_msg=k)


def test_record_wraps_and_matches_push_twin():
    from porl_amd.buffer.replay_buffer import ReplayBuffer
    S, cap = 6, 37
    a, b = ReplayBuffer(cap, (S,), DEV), ReplayBuffer(cap, (S,), DEV)
    np.random.seed(0)
    for i, tr in enumerate(_transitions(3 * cap + 5, S, seed=1)):
        assert a.record(*tr)
        b.push(*tr)
        if i % 9 == 8:
            idx = np.random.choice(a.size, 8, replace=False)
            ga, gb = a.sample_at(idx), b.sample_at(idx)
            for x, y in zip(ga, gb):
                assert torch.equal(x, y)
    assert a._pending == []
    b._sync_mirror()
    assert (a.size, a.position) == (b.size, b.position) == (cap, (3 * cap + 5) % cap)
    for k in ("states", "actions", "rewards", "next_states", "dones"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
        assert torch.equal(a._mirror[k], b._mirror[k])
    _assert_mirror_is_host(a)


def test_record_many_without_sync():
    from porl_amd.buffer.replay_buffer import ReplayBuffer
    S = 8
    rb = ReplayBuffer(256, (S,), DEV)
    trs = _transitions(200, S, seed=2)
    rb.record(*trs[0])                                          # creates the mirror
    for tr in trs[1:]:
        rb.record(*tr)                                          # 199 launches, nothing waits in between
    torch.cuda.synchronize()
    _assert_mirror_is_host(rb)
    np.testing.assert_array_equal(rb.states[:200], np.stack([t[0] for t in trs]))


def test_record_at_the_widest_state():
    from porl_amd.buffer.replay_buffer import ReplayBuffer
    from porl_amd.train.cql_trainer import QnetEngine
    S = QnetEngine.RECORD_MAX_STATE
    rb = ReplayBuffer(5, (S,), DEV)
    for tr in _transitions(7, S, seed=3):
        assert rb.record(*tr)
    _assert_mirror_is_host(rb)
    wide = ReplayBuffer(5, (S + 1,), DEV)
    wide.record(*_transitions(1, S + 1, seed=4)[0])             # creates the mirror
    assert not wide.record(*_transitions(1, S + 1, seed=5)[0])  # too wide for the arguments: push's deferred path
    wide._sync_mirror()
    _assert_mirror_is_host(wide)


# -- fast path against the reference loop on the same trainer ----------------------------------------------------------
def _run(make, fast, seed=7, episodes=4, max_steps=30):
    from porl_amd.train import online
    t = make()
    t.logger = RecordingLogger()
    if fast:
        t.select_action = _refuse                              # the one-launch path never calls it
    env = ToyEnv(seed=seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    orig = online.fast_ok
    if not fast:
        online.fast_ok = lambda trainer: False
    try:
        rewards = _quiet(t.train_online, env, num_episodes=episodes, max_steps=max_steps)
    finally:
        online.fast_ok = orig
    return t, env, rewards


@pytest.mark.parametrize("which", ["dddqn", "dqn_wide", "cql", "qr"])
def test_fast_path_equals_reference_loop(which):
    from porl_amd.net.q_network import QNetwork
    from porl_amd.train.cql_trainer import CQLTrainer
    from porl_amd.train.dddqn_trainer import DDDQNTrainer
    from porl_amd.train.dqn_trainer import DQNTrainer
    from porl_amd.train.qr_dqn_trainer import QRDQNTrainer
    kw = dict(epsilon=1.0, epsilon_min=0.05, epsilon_decay=0.5, update_target_freq=2, device=DEV, batch_size=16)

    def make():
        torch.manual_seed(0)
        if which == "dddqn":
            return DDDQNTrainer(8, 4, 0.99, transition_learning_step=20, **kw)
        if which == "dqn_wide":                                # not on the one-launch step kernel: gather + multi-launch
            return DQNTrainer(8, 4, 0.99, transition_learning_step=20, network=lambda s, a: QNetwork(s, a, [256, 256]), **kw)
        if which == "cql":
            return CQLTrainer(8, 4, 0.99, transition_learning_step=20, **kw)
        return QRDQNTrainer(8, 4, 0.99, num_quantiles=12, network_hidden_sizes=[64, 64], transition_learning_step=20, **kw)
    a, env_a, ra = _run(make, True)
    b, env_b, rb_ = _run(make, False)
    assert env_a.actions == env_b.actions and ra == rb_
    la = [c for c in a.logger.calls]
    lb = [c for c in b.logger.calls]
    assert [c[:3] + (c[4] is None,) if c[0] == "log_step" else c[:2] for c in la] == \
           [c[:3] + (c[4] is None,) if c[0] == "log_step" else c[:2] for c in lb]
    loss_a = [c[4] for c in la if c[0] == "log_step" and c[4] is not None]
    loss_b = [c[4] for c in lb if c[0] == "log_step" and c[4] is not None]
    assert len(loss_a) > 20
    np.testing.assert_allclose(loss_a, loss_b, rtol=1e-5, atol=1e-7)
    for x, y in zip(a.q_network.parameters(), b.q_network.parameters()):
        np.testing.assert_allclose(x.detach().cpu().numpy(), y.detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert a.replay_buffer._pending == []
    _assert_mirror_is_host(a.replay_buffer)


def test_async_losses_reach_the_logger_as_device_statistics():
    from porl_amd.train.dqn_trainer import DQNTrainer
    t = DQNTrainer(8, 4, 0.99, epsilon_decay=0.5, update_target_freq=2, device=DEV, batch_size=16, transition_learning_step=20)
    t.async_losses = True
    t.logger = RecordingLogger()
    np.random.seed(0)
    _quiet(t.train_online, ToyEnv(seed=1), num_episodes=2, max_steps=30)
    losses = [c[4] for c in t.logger.calls if c[0] == "log_step" and c[4] is not None]
    assert losses and all(isinstance(v, torch.Tensor) and v.device.type == "cuda" for v in losses)


# -- loop semantics off the fast path ---------------------------------------------------------------------------------
class _Counter:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return 0.125 * self.n


def _check_semantics(t, threshold, episodes=4, max_steps=30):
    log = t.logger = RecordingLogger()
    orig_sync = t.sync_target
    t.sync_target = lambda: (log.calls.append(("sync",)), orig_sync())
    pol = _Counter()
    env = ToyEnv(seed=9)
    eps0, decay, eps_min = t.epsilon, t.epsilon_decay, t.epsilon_min
    np.random.seed(9)
    rewards = _quiet(t.train_online, env, pol, num_episodes=episodes, max_steps=max_steps)
    assert env.closed and log.calls[-1] == ("close",)
    # the expected call sequence, from the episode lengths the environment saw
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


@pytest.fixture(autouse=True)
def _track_episode_lengths(monkeypatch):
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


def test_per_train_online_semantics():
    from porl_amd.train.dqn_per_trainer import PERTrainer
    t = PERTrainer(8, 4, 0.99, epsilon=1.0, epsilon_decay=0.5, update_target_freq=2, device=DEV, batch_size=24)
    _check_semantics(t, threshold=24)                          # len(memory) >= batch_size (dqn_per_trainer.py:154)
    assert len(t.memory) > 24 and len(t.replay_buffer) == 0    # memory.add, not replay_buffer.push


def test_iqn_train_online_semantics():
    from porl_amd.train.iqn_trainer import IQNTrainer
    assert IQNTrainer(8, 4, 0.99, device=DEV, hidden_size=32).training_learning_step == 10000
    t = IQNTrainer(8, 4, 0.99, epsilon=1.0, epsilon_decay=0.5, update_target_freq=3, device=DEV, hidden_size=32,
                   transition_learning_step=30)
    _check_semantics(t, threshold=30)


def test_dddqn_train_online_semantics():
    from porl_amd.train.dddqn_trainer import DDDQNTrainer
    t = DDDQNTrainer(8, 4, 0.99, epsilon=1.0, epsilon_decay=0.5, update_target_freq=2, device=DEV, transition_learning_step=17)
    _check_semantics(t, threshold=17)


def test_iqn_train_offline_logs_every_loss():
    from porl_amd.train.iqn_trainer import IQNTrainer
    t = IQNTrainer(8, 4, 0.99, device=DEV, hidden_size=32, batch_size=16, update_target_freq=2)
    for tr in _transitions(64, 8, seed=6):
        t.replay_buffer.push(tr[0], tr[1] % 4, tr[2], tr[3], tr[4])
    t.logger = RecordingLogger()
    np.random.seed(1)
    losses = t.train_offline(num_iterations=4)
    assert t.training_step == 3
    assert t.logger.calls == [("log_loss", i, losses[i]) for i in range(4)] + [("close",)]
