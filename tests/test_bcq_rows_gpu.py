"""Discrete BCQ from one native call per step (csrc/bcq_mask.hpp, porl_qnet_bcq_*): the behaviour-mask kernel against an
fp64 oracle and against BehaviorPolicy.sample, its exact cases, bcq_learn_rows against the existing pieces and the
reference's golden run, the device-sampled forms against the indexed ones, and BCQTrainer.train(policy=bcq_learn) against
the reference's own online loop (scripts/gen_golden_online_bcq.py)."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from helpers import bcq_cases
from helpers.online_env import RecordingLogger, ToyEnv
from porl_amd import _native as N
from porl_amd.util.synth import make_discrete_transitions

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _np_sd(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _refuse(*a, **k):
    raise AssertionError("train_online left its one-launch path")


def _behaviour(S, A, hidden, params, max_batch=128):
    """A BehaviorPolicy on an engine of its own, as BCQTrainer attaches it."""
    from porl_amd.net.behavior_policy import BehaviorPolicy
    from porl_amd.train.cql_trainer import QnetEngine
    bp = BehaviorPolicy(S, A, hidden_sizes=hidden)
    eng = QnetEngine(S, A, hidden, max_batch, DEV)
    with torch.no_grad():
        for p, v in zip(bp.parameters(), eng.views(eng.params)):
            p.data = v
    bp._engine = eng
    bp.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return bp, eng


# -- the mask kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden_key", list(bcq_cases.HIDDEN))
def test_mask_matches_fp64_oracle_and_behavior_policy_sample(hidden_key):
    SENTINEL = -7.0
    n_bad = 0
    for B, A, S in bcq_cases.shapes(hidden_key):
        case = bcq_cases.make(hidden_key, B, A, S)
        bp, eng = _behaviour(S, A, case["hidden"], case["params"])
        assert eng.fused == (hidden_key != "wide")                   # [256]: the multi-launch fallback
        want, clear = bcq_cases.decided(case)
        ns = torch.from_numpy(case["next_states"]).to(DEV)
        idx = torch.from_numpy(case["idx"]).to(DEV)
        out = torch.full((B * A + 96,), SENTINEL, dtype=torch.float32, device=DEV)
        got = eng.bcq_mask(ns, idx, case["threshold"], out=out)
        assert got.data_ptr() == out.data_ptr()
        flat = out.cpu().numpy()
        got = flat[:B * A].reshape(B, A)
        assert (flat[B * A:] == SENTINEL).all(), (B, A, S)            # rows past B of the last block write nothing
        assert set(np.unique(got)) <= {0.0, 1.0}
        n_bad += int((~clear).sum())
        np.testing.assert_array_equal(got[clear], want[clear], err_msg=str((B, A, S)))
        old = bp.sample(ns[idx], case["threshold"]).cpu().numpy()
        np.testing.assert_array_equal(got[clear], old[clear], err_msg=str((B, A, S)))
    print(f"{hidden_key}: {n_bad} entries within {bcq_cases.MARGIN} of the threshold were left out")


@pytest.mark.parametrize("threshold,want", [(0.5, 0.0), (float(np.nextafter(np.float32(0.5), np.float32(0))), 1.0)])
def test_mask_comparison_is_strict(threshold, want):
    """All-zero behaviour parameters, A = 2: every probability is exactly 0.5 — not above 0.5, above the float below it."""
    S, A, B = 10, 2, 33
    params = {k: np.zeros_like(v) for k, v in bcq_cases.make("default", B, A, S)["params"].items()}
    bp, eng = _behaviour(S, A, [64, 128], params)
    ns = torch.randn(50, S, device=DEV)
    idx = torch.randperm(50, device=DEV)[:B]
    got = eng.bcq_mask(ns, idx, threshold).cpu().numpy()
    np.testing.assert_array_equal(got, np.full((B, A), want, dtype=np.float32))


# -- bcq_learn_rows ---------------------------------------------------------------------------------------------------
def _filled(t, N_, S, A, seed, capacity=None):
    st, ac, rw, ns, dn = make_discrete_transitions(N_, S, A, seed=seed)
    t.replay_buffer = type(t.replay_buffer)(capacity or N_, (S,), DEV)
    for i in range(N_):
        t.replay_buffer.push(st[i], int(ac[i]), float(rw[i]), ns[i], bool(dn[i]))
    return st, ac, rw, ns, dn


def test_rows_with_no_allowed_action_fall_back_to_the_first_action():
    """threshold = 1.0: no action passes, every masked value ties at -1e10 and torch.argmax returns index 0
    (bcq.py:68-73) — computed as tests/test_cql_gpu.py does for bcq_learn."""
    from porl_amd.policy.bcq import bcq_learn_rows
    from porl_amd.train.bcq_trainer import BCQTrainer
    S, A, B, N_ = 8, 5, 32, 64
    torch.manual_seed(0)
    t = BCQTrainer(S, A, 0.9, device=DEV, batch_size=B, threshold=1.0)
    st, ac, rw, ns, dn = _filled(t, N_, S, A, 2)
    idx = np.random.default_rng(0).permutation(N_)[:B]
    tq = t.target_network(torch.from_numpy(ns[idx]).to(DEV)).cpu().numpy()
    q = t.q_network(torch.from_numpy(st[idx]).to(DEV)).cpu().numpy()
    loss = bcq_learn_rows(t, torch.from_numpy(idx).to(DEV))
    y = rw[idx] + 0.9 * tq[:, 0] * (1 - dn[idx])
    want = np.mean((q[np.arange(B), ac[idx]] - y) ** 2)
    assert isinstance(loss, float)
    np.testing.assert_allclose(loss, want, rtol=2e-5)


def _pair(network, B, threshold=0.17, S=10, A=6, N_=200, capacity=None, **kw):
    from porl_amd.train.bcq_trainer import BCQTrainer
    out = []
    for _ in range(2):
        torch.manual_seed(3)
        t = BCQTrainer(S, A, 0.97, device=DEV, batch_size=B, threshold=threshold, network=network, **kw)
        with torch.no_grad():                                          # a target network of its own, as after training
            g = torch.Generator().manual_seed(4)
            for p in t.target_network.parameters():
                p.add_((0.05 * torch.randn(p.shape, generator=g)).to(DEV))
            for p in t.behavior_policy.parameters():
                p.mul_(3.0)                                            # spread the probabilities around the threshold
        if t._dueling is not None:
            t._dueling.compose(1)
        _filled(t, N_, S, A, 5, capacity)
        out.append(t)
    return out


def _existing_step(t, idx):
    """The pieces bcq_learn runs today, on the gathered rows."""
    from porl_amd.policy import bcq
    batch = t.replay_buffer.gather_device(idx)
    mask = t.behavior_policy.sample(batch[3], t.threshold)
    var = N.QnetVariant(0, None, None, None, mask.data_ptr(), 0)
    stats = bcq._step(t, t._engine, t.optimizer, batch, 0.0, var)
    return float(stats[0]), mask


def _same_q(a, b):
    for (k, x), (_, y) in zip(a.q_network.state_dict().items(), b.q_network.state_dict().items()):
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=k)


@pytest.mark.parametrize("B", [64, 40])
@pytest.mark.parametrize("net", ["qnetwork", "dueling", "wide"])
def test_rows_path_equals_the_existing_pieces(net, B):
    from porl_amd.net.q_network import DuelingQNetwork, QNetwork
    from porl_amd.policy.bcq import bcq_learn_rows
    network = {"qnetwork": QNetwork, "dueling": DuelingQNetwork, "wide": lambda s, a: QNetwork(s, a, [256, 64])}[net]
    a, b = _pair(network, B)
    assert a._engine.fused == (net != "wide") and a._behavior_engine.fused
    rng = np.random.default_rng(B)
    a.replay_buffer._sync_mirror()
    b.replay_buffer._sync_mirror()
    seen = []
    for k in range(5):
        idx = torch.from_numpy(rng.permutation(200)[:B]).to(DEV)
        la = bcq_learn_rows(a, idx)
        lb, mask = _existing_step(b, idx)
        seen.append(float(mask.mean()))
        np.testing.assert_allclose(la, lb, rtol=1e-5, atol=1e-6, err_msg=f"step {k}")
    assert 0.1 < np.mean(seen) < 0.9                                 # the mask really selects
    assert a.optimizer.step_count == b.optimizer.step_count == 5
    _same_q(a, b)


def test_rows_path_matches_reference_golden():
    """tests/test_cql_gpu.py's BCQ golden, the learn steps through bcq_learn_rows on numpy's own draws."""
    from porl_amd.policy.bcq import bcq_behavior_pretrain, bcq_learn_rows
    from porl_amd.train.bcq_trainer import BCQTrainer
    z, _ = load_golden("bcq_s10_a6")
    S, A, B, K, N_, seed_model, seed_data, seed_np, KP = (int(v) for v in z["meta"])
    torch.manual_seed(seed_model)
    t = BCQTrainer(S, A, float(z["gamma"]), device=DEV, batch_size=B, num_epochs=KP, threshold=float(z["threshold"]))
    t.behavior_policy.load_state_dict({k: torch.from_numpy(v) for k, v in sub(z, "init_behavior/").items()})
    t.q_network.load_state_dict({k: torch.from_numpy(v) for k, v in sub(z, "init/").items()})
    t.target_network.load_state_dict({k: torch.from_numpy(v) for k, v in sub(z, "init_target/").items()})
    _filled(t, N_, S, A, seed_data)
    np.random.seed(seed_np)
    np.testing.assert_allclose(bcq_behavior_pretrain(t), z["ce_loss"], rtol=2e-5)
    for k in range(K):
        idx = torch.from_numpy(np.random.choice(N_, B, replace=False)).to(DEV)
        np.testing.assert_allclose(bcq_learn_rows(t, idx), z["loss"][k], rtol=2e-5)
    got = _np_sd(t.q_network)
    for k, v in sub(z, "final/").items():
        np.testing.assert_allclose(got[k], v, atol=1e-5, err_msg=k)


# -- device-sampled ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,capacity", [(200, 200), (200, 333)])
def test_device_sampled_learn_equals_rows_on_the_same_draws(n_rows, capacity):
    from porl_amd import engine as E
    from porl_amd.net.q_network import QNetwork
    from porl_amd.policy.bcq import bcq_learn_device_sampled, bcq_learn_rows
    B, seed = 64, 11
    a, b = _pair(QNetwork, B, N_=n_rows, capacity=capacity)
    assert a._engine.can_sample and a.replay_buffer.size == n_rows and a.replay_buffer.capacity == capacity
    for draw in range(4):
        la = bcq_learn_device_sampled(a, seed)
        b.replay_buffer._sync_mirror()
        idx = E.sample_indices(n_rows, B, seed, draw, device=DEV)
        assert int(idx.max()) < n_rows and len(set(idx.tolist())) == B
        np.testing.assert_allclose(la, bcq_learn_rows(b, idx), rtol=1e-5, atol=1e-6, err_msg=f"draw {draw}")
    assert a._draws == 4
    _same_q(a, b)
    a.async_losses = True
    out = bcq_learn_device_sampled(a, seed)
    assert isinstance(out, torch.Tensor) and out.device.type == "cuda" and out.numel() == 3 and a._draws == 5


def test_device_sampled_learn_with_a_wide_behaviour_network():
    """A Q engine that samples in the kernel beside a behaviour network the mask kernel does not cover ([256]): the mask
    side draws the same rows with the sampler kernel into its staging space, gathers and runs the multi-launch forward."""
    from porl_amd import engine as E
    from porl_amd.net.behavior_policy import BehaviorPolicy
    from porl_amd.net.q_network import QNetwork
    from porl_amd.policy.bcq import bcq_learn_device_sampled, bcq_learn_rows
    B, seed, n_rows = 40, 9, 200
    a, b = _pair(QNetwork, B, N_=n_rows, capacity=256, behavior_policy=lambda s, a_: BehaviorPolicy(s, a_, [256]))
    assert a._engine.can_sample and not a._behavior_engine.fused
    for draw in range(3):
        la = bcq_learn_device_sampled(a, seed)
        b.replay_buffer._sync_mirror()
        idx = E.sample_indices(n_rows, B, seed, draw, device=DEV)
        lb, mask = _existing_step(b, idx)
        assert 0.05 < float(mask.mean()) < 0.95
        np.testing.assert_allclose(la, lb, rtol=1e-5, atol=1e-6, err_msg=f"draw {draw}")
    _same_q(a, b)
    # ... and the indexed call on the same fallback
    idx = E.sample_indices(n_rows, B, seed, 7, device=DEV)
    np.testing.assert_allclose(bcq_learn_rows(a, idx), _existing_step(b, idx)[0], rtol=1e-5, atol=1e-6)


def test_sampled_calls_are_unsupported_without_in_kernel_sampling():
    """A Q / behaviour engine off the two-group step kernel: the sampled entry points answer PORL_ERR_UNSUPPORTED (-2) and
    launch nothing; the Python forms route around them (sample_indices + the indexed call)."""
    from porl_amd import engine as E
    from porl_amd.net.behavior_policy import BehaviorPolicy
    from porl_amd.net.q_network import QNetwork
    from porl_amd.policy import bcq
    B, n_rows = 40, 200
    a, b = _pair(lambda s, a_: QNetwork(s, a_, [256, 64]), B, N_=n_rows, num_epochs=3,
                 behavior_policy=lambda s, a_: BehaviorPolicy(s, a_, [256]))
    eng, beh, m = a._engine, a._behavior_engine, a.replay_buffer
    m._sync_mirror()
    m = m._mirror
    assert not eng.can_sample and not beh.can_sample
    before = eng.params.clone(), beh.params.clone()
    hp = eng.hyper(0.97, 0.0, 1.0 / B, 1, 5e-4)
    args = (m["states"], m["actions"], m["rewards"], m["next_states"], m["dones"])
    with pytest.raises(N.NativeError, match=r"rc=-2"):
        eng.bcq_learn_sampled(beh, hp, *args, n_rows, B, 0, 0, 0.17)
    with pytest.raises(N.NativeError, match=r"rc=-2"):
        beh.learn_sampled(hp, *args, n_rows, B, 0, 0, variant=N.QnetVariant(0, None, None, None, None, 1))
    torch.cuda.synchronize()
    assert torch.equal(eng.params, before[0]) and torch.equal(beh.params, before[1])
    # the Python forms take the indexed route and equal the existing pieces on the same draws
    la = bcq.bcq_learn_device_sampled(a, 3)
    b.replay_buffer._sync_mirror()
    lb, _ = _existing_step(b, E.sample_indices(n_rows, B, 3, 0, device=DEV))
    np.testing.assert_allclose(la, lb, rtol=1e-5, atol=1e-6)
    got = bcq.bcq_pretrain_device_sampled(a, 3)
    var = N.QnetVariant(0, None, None, None, None, 1)
    want = [float(bcq._step(b, b._behavior_engine, b.behavior_optimizer,
                            b.replay_buffer.gather_device(E.sample_indices(n_rows, B, 3, d, device=DEV)), 1.0, var)[2])
            + math.log(b.action_size) for d in range(1, 4)]
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("n_rows,capacity", [(200, 200), (200, 333)])
def test_device_sampled_pretrain_equals_the_step_on_the_same_draws(n_rows, capacity):
    from porl_amd import engine as E
    from porl_amd.net.q_network import QNetwork
    from porl_amd.policy import bcq
    B, seed, KP = 64, 5, 6
    a, b = _pair(QNetwork, B, N_=n_rows, capacity=capacity, num_epochs=KP)
    got = bcq.bcq_pretrain_device_sampled(a, seed)
    assert len(got) == KP and all(isinstance(v, float) for v in got)
    b.replay_buffer._sync_mirror()
    var = N.QnetVariant(0, None, None, None, None, 1)
    want = []
    for draw in range(KP):
        idx = E.sample_indices(n_rows, B, seed, draw, device=DEV)
        stats = bcq._step(b, b._behavior_engine, b.behavior_optimizer, b.replay_buffer.gather_device(idx), 1.0, var)
        want.append(float(stats[2]) + math.log(b.action_size))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    assert want[-1] < want[0]                                        # the cross-entropy falls
    for (k, x), (_, y) in zip(a.behavior_policy.state_dict().items(), b.behavior_policy.state_dict().items()):
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=k)


# -- online -----------------------------------------------------------------------------------------------------------
def _golden_trainer(z, rb_cls=None):
    from porl_amd.buffer.replay_buffer import ReplayBuffer
    from porl_amd.train.bcq_trainer import BCQTrainer
    S, A, EP, MS, THR, B, TF, CAP, seed_env, seed_np, prefill, epochs, seed_data = (int(v) for v in z["meta"])
    eps, eps_min, decay, gamma = (float(v) for v in z["eps"])
    rb = (rb_cls or ReplayBuffer)(CAP, (S,), DEV)
    t = BCQTrainer(S, A, gamma, eps, eps_min, decay, TF, DEV, batch_size=B, replay_buffer=rb, transition_learning_step=THR,
                   num_epochs=epochs, threshold=float(z["threshold"]))
    init = {k: torch.from_numpy(v) for k, v in sub(z, "init/").items()}
    t.q_network.load_state_dict(init)
    t.target_network.load_state_dict(init)
    t.behavior_policy.load_state_dict({k: torch.from_numpy(v) for k, v in sub(z, "init_behavior/").items()})
    for i in range(prefill):
        rb.push(z["prefill/states"][i], int(z["prefill/actions"][i]), float(z["prefill/rewards"][i]),
                z["prefill/next_states"][i], bool(z["prefill/dones"][i]))
    t.logger = RecordingLogger()
    return t, EP, MS, seed_env, seed_np


def _train(t, z, EP, MS, seed_env, seed_np):
    from porl_amd.policy.bcq import bcq_behavior_pretrain, bcq_learn
    env = ToyEnv(seed=seed_env)
    np.random.seed(seed_np)
    rewards = _quiet(t.train, env=env, policy=bcq_learn, num_episodes=EP, max_steps=MS, pretrain=bcq_behavior_pretrain)
    calls = [c for c in t.logger.calls if c[0] in ("log_step", "log_episode")]
    losses = [c[4] for c in calls if c[0] == "log_step" and c[4] is not None]
    return env, rewards, calls, losses


def test_train_with_bcq_learn_matches_reference_golden():
    """BCQTrainer.train(env, policy=bcq_learn, pretrain=bcq_behavior_pretrain) — the script's call, which raised TypeError
    — against the reference's pre-training followed by its online loop with bcq_learn bound to the trainer."""
    z, _ = load_golden("online_bcq_s8_a4")
    assert float(z["min_gap"]) > 1e-3 and float(z["min_margin"]) >= 1e-4
    t, EP, MS, seed_env, seed_np = _golden_trainer(z)
    t.select_action = _refuse                                        # the fast path never calls them
    t.get_action = _refuse
    env, rewards, calls, losses = _train(t, z, EP, MS, seed_env, seed_np)
    got = _np_sd(t.behavior_policy)
    for k, v in sub(z, "behavior_after/").items():
        np.testing.assert_allclose(got[k], v, rtol=1e-4, atol=2e-6, err_msg=k)
    np.testing.assert_array_equal(np.array(env.actions), z["actions"])
    np.testing.assert_array_equal(np.array(rewards, dtype=np.float64), z["rewards_history"])
    assert t.epsilon == float(z["final_epsilon"])
    log = np.array([[0, c[1], c[2], c[4] is not None] if c[0] == "log_step" else [1, c[1], -1, 0] for c in calls])
    np.testing.assert_array_equal(log, z["log_calls"])
    assert t.logger.calls[-1] == ("close",) and env.closed
    assert all(isinstance(v, float) for v in losses)
    np.testing.assert_allclose(losses, z["losses"], rtol=1e-4, atol=1e-7)
    for pre, mod in (("final/", t.q_network), ("final_target/", t.target_network)):
        want, have = sub(z, pre), _np_sd(mod)
        assert list(have) == list(want)
        for k in want:
            np.testing.assert_allclose(have[k], want[k], rtol=1e-4, atol=2e-6, err_msg=pre + k)
    rb = t.replay_buffer
    assert rb.position == int(z["buf/position"])
    for k in ("states", "actions", "rewards", "next_states", "dones"):
        np.testing.assert_array_equal(getattr(rb, k)[:rb.size], z["buf/" + k], err_msg=k)


def test_train_off_the_fast_path_runs_the_reference_loop_to_the_same_losses():
    """A replay buffer the one-launch path does not know (a subclass): the reference loop with `lambda: bcq_learn(self)`."""
    from porl_amd.buffer.replay_buffer import ReplayBuffer
    from porl_amd.train import online

    class ElsewhereBuffer(ReplayBuffer):
        pass
    z, _ = load_golden("online_bcq_s8_a4")
    t, EP, MS, seed_env, seed_np = _golden_trainer(z, ElsewhereBuffer)
    assert not online.fast_ok(t)
    used = []
    act = t.select_action
    t.select_action = lambda s: (used.append(1), act(s))[1]
    env, rewards, calls, losses = _train(t, z, EP, MS, seed_env, seed_np)
    assert len(used) == len(z["actions"])                             # the trainer's own action rule ran every step
    np.testing.assert_array_equal(np.array(env.actions), z["actions"])
    np.testing.assert_allclose(losses, z["losses"], rtol=1e-4, atol=1e-7)


def test_train_online_without_policy_still_runs_plain_learn():
    z, _ = load_golden("online_bcq_s8_a4")
    t, EP, MS, seed_env, seed_np = _golden_trainer(z)
    n = []
    learn = t._learn_rows
    t._learn_rows = lambda idx: (n.append(1), learn(idx))[1]
    np.random.seed(seed_np)
    _quiet(t.train_online, ToyEnv(seed=seed_env), num_episodes=2, max_steps=MS)
    losses = [c[4] for c in t.logger.calls if c[0] == "log_step" and c[4] is not None]
    assert len(n) == len(losses) > 10 and t.behavior_optimizer.step_count == 0
    for k, v in sub(z, "init_behavior/").items():                    # the behaviour policy was never touched
        np.testing.assert_array_equal(_np_sd(t.behavior_policy)[k], v)
