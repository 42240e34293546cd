"""The offline half in the discrete lidar task on the device (porl_amd/train/vector_offline.py, evaluate.evaluate_discrete):
collect, learn and score, each against a hand-written loop of the public calls it is made of.  Everything is an identity:
the same kernels with the same arguments in the same order leave the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
A, B, EP_STEP, SEED = 5, 32, 20, 7


def make_sim(n=64, n_beams=20, auto_reset=True, **kw):
    from porl_amd.env import DiscreteLidarNavSim, NavWorld
    kw = dict(dict(n_actions=A, seed=3, env_offset=5, auto_reset=auto_reset, n_beams=n_beams, episode_step=EP_STEP), **kw)
    return DiscreteLidarNavSim(NavWorld.lattice(), n, **kw)


def make_trainer(kind, tmp_path, S=22, q_hidden=(64, 64), **kw):
    from porl_amd.net.q_network import QNetwork
    torch.manual_seed(0)
    common = dict(dict(device=DEV, batch_size=B, log_dir=str(tmp_path), update_target_freq=3), **kw)
    net = lambda s, a: QNetwork(s, a, list(q_hidden))
    if kind == "dqn":
        from porl_amd.train.dqn_trainer import DQNTrainer
        return DQNTrainer(S, A, 0.99, network=net, **common)
    if kind == "ddqn":
        from porl_amd.train.dqn_trainer import DDQNTrainer
        return DDQNTrainer(S, A, 0.99, network=net, **common)
    if kind == "cql":
        from porl_amd.train.cql_trainer import CQLTrainer
        return CQLTrainer(S, A, 0.99, network=net, alpha=0.5, **common)
    if kind == "bcq":
        from porl_amd.train.bcq_trainer import BCQTrainer
        return BCQTrainer(S, A, 0.99, network=net, threshold=0.2, num_epochs=5, **common)
    if kind == "per":
        from porl_amd.train.dqn_per_trainer import PERTrainer
        return PERTrainer(S, A, 0.99, capacity=256, **common)
    if kind == "c51":
        from porl_amd.train.c51_trainer import C51Trainer
        return C51Trainer(S, A, 0.99, atom_size=11, network_hidden_sizes=[64, 64], **common)
    if kind == "qr":
        from porl_amd.train.qr_dqn_trainer import QRDQNTrainer
        return QRDQNTrainer(S, A, 0.99, num_quantiles=12, network_hidden_sizes=[64, 64], **common)
    from porl_amd.train.iqn_trainer import IQNTrainer
    return IQNTrainer(S, A, 0.99, embedding_dim=10, hidden_size=32, num_quantiles_n_policy=6, num_quantiles_n_prime_loss=3,
                      num_quantiles_n_double_prime_loss=5, buffer_size=64, **common)


def trainer_state(t):
    """Every tensor and counter of a trainer that learning or acting could move."""
    if hasattr(t, "_engine"):
        engines = [t._engine] + ([t._behavior_engine] if hasattr(t, "_behavior_engine") else [])
        tensors = [getattr(e, name).clone() for e in engines for name in ("params", "params_tgt", "adam_m", "adam_v")]
        steps = [t.optimizer.step_count] + ([t.behavior_optimizer.step_count] if hasattr(t, "behavior_optimizer") else [])
    else:                                                                       # IQN: the flat buffers of its optimizers
        o = t.optimizer
        tensors = [x.clone() for x in (o.flat, t._target.flat, o.exp_avg, o.exp_avg_sq)]
        steps = [o.step_count]
    scalars = (t.epsilon, steps, getattr(t, "_draws", None), getattr(t, "_vec_steps", None), len(getattr(t, "replay_buffer", ())),
               getattr(t, "device_replay", None))
    return tensors, scalars


def assert_state_equal(a, b):
    assert a[1] == b[1], (a[1], b[1])
    assert len(a[0]) == len(b[0])
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), k


def replay_state(r):
    return [x.clone() for x in r.arrays()], (r.position, r.size)


# ---- collect ------------------------------------------------------------------------------------------------------------------
def test_collect_random_equals_a_hand_loop_of_qnet_select_and_step():
    from porl_amd import engine as E
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.train.vector_offline import collect_discrete
    n, steps = 96, 25                                          # 2400 rows into 1000 slots: the ring wraps
    sim, replay = make_sim(n, 36), DeviceReplay(1000, 38, DEV)
    out = collect_discrete(sim, replay, steps, seed=SEED, t0=4)
    sim2, replay2 = make_sim(n, 36), DeviceReplay(1000, 38, DEV)
    sim2.reset()
    dummy = torch.zeros(n, A, device=DEV)
    for k in range(steps):
        sim2.step(E.qnet_select(dummy, 1.0, SEED, 4 + k, env_offset=sim2.env_offset), replay=replay2)
    got, want = replay_state(replay), replay_state(replay2)
    assert got[1] == want[1] == (2400 % 1000, 1000)
    for x, y in zip(got[0], want[0]):
        assert torch.equal(x, y)
    assert torch.equal(sim.state, sim2.state) and torch.equal(sim.counters, sim2.counters) and torch.equal(sim.obs, sim2.obs)
    assert out["transitions"] == 2400 and np.array_equal(out["tallies"], sim2.tallies.sum(0).cpu().numpy())
    assert out["tallies"][0] >= n                              # 25 steps of 20-step episodes: every robot finished one
    assert set(replay.actions.cpu().numpy().tolist()) == set(range(A))
    # a second call continues the first when t0 moves on
    sim3, replay3 = make_sim(n, 36), DeviceReplay(1000, 38, DEV)
    collect_discrete(sim3, replay3, 10, seed=SEED, t0=4)
    collect_discrete(sim3, replay3, 15, seed=SEED, t0=14)
    for x, y in zip(replay_state(replay3)[0], got[0]):
        assert torch.equal(x, y)


def test_collect_with_a_trainer_equals_a_hand_loop_of_act_rows_and_step(tmp_path):
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.train.vector_offline import collect_discrete
    t = make_trainer("dqn", tmp_path)
    before = trainer_state(t)
    sim, replay = make_sim(64, 20), DeviceReplay(2000, 22, DEV)
    out = collect_discrete(sim, replay, 12, trainer=t, epsilon=0.3, seed=SEED)
    assert_state_equal(before, trainer_state(t))               # the trainer is read, not modified
    assert t.epsilon == 1.0
    sim2, replay2 = make_sim(64, 20), DeviceReplay(2000, 22, DEV)
    sim2.reset()
    for k in range(12):
        sim2.step(t._engine.act_rows(sim2.obs, 0.3, SEED, k, env_offset=sim2.env_offset), replay=replay2)
    assert (replay.position, replay.size) == (replay2.position, replay2.size) == (768, 768) and out["transitions"] == 768
    for x, y in zip(replay.arrays(), replay2.arrays()):
        assert torch.equal(x, y)
    # not the random policy: the greedy share shows
    sim3, replay3 = make_sim(64, 20), DeviceReplay(2000, 22, DEV)
    collect_discrete(sim3, replay3, 12, seed=SEED)
    assert not torch.equal(replay.actions, replay3.actions)
    # every family has its act call here
    for kind in ("bcq", "c51", "qr", "iqn"):
        tk = make_trainer(kind, tmp_path)
        rk = DeviceReplay(200, 22, DEV)
        assert collect_discrete(make_sim(64, 20), rk, 2, trainer=tk, epsilon=0.5, seed=SEED)["transitions"] == 128 == len(rk)


def test_collect_refusals(tmp_path):
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.train.vector_offline import collect_discrete
    t = make_trainer("dqn", tmp_path)
    replay = DeviceReplay(200, 22, DEV)
    for tr in (None, t):
        with pytest.raises(ValueError, match="auto_reset"):
            collect_discrete(make_sim(auto_reset=False), replay, 2, trainer=tr)
    with pytest.raises(ValueError, match="observes"):
        collect_discrete(make_sim(n_beams=36), DeviceReplay(200, 38, DEV), 2, trainer=t)
    with pytest.raises(ValueError, match="n_steps"):
        collect_discrete(make_sim(), replay, 0)
    with pytest.raises(ValueError, match="replay"):
        collect_discrete(make_sim(), DeviceReplay(200, 38, DEV), 2)
    assert len(replay) == 0


# ---- learn --------------------------------------------------------------------------------------------------------------------
def filled_replay(seed=SEED):
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.train.vector_offline import collect_discrete
    replay = DeviceReplay(600, 22, DEV)
    collect_discrete(make_sim(64, 20), replay, 8, seed=seed)   # 512 rows of the random policy
    return replay


@pytest.mark.parametrize("q_hidden", [(64, 64), (160, 64)])
def test_train_offline_device_bcq_equals_the_engine_calls(q_hidden, tmp_path):
    """Pre-training and learn steps against the explicit sequence of public engine calls with the same draws and sync
    schedule; Q hidden [160, 64] is off the one-launch plan (no in-kernel sampling: sample_indices + the indexed forms)."""
    from porl_amd import _native as N
    from porl_amd import engine as E
    replay = filled_replay()
    ta, tb = make_trainer("bcq", tmp_path, q_hidden=q_hidden), make_trainer("bcq", tmp_path, q_hidden=q_hidden)
    assert ta._engine.fused == (q_hidden == (64, 64)) and (ta._engine.fused or not ta._engine.can_sample)
    ta._draws = tb._draws = 2                                  # the counter is shared with the other device-sampled calls
    out = ta.train_offline_device(replay, 7, seed=SEED)
    assert out["learn_steps"] == 7 and len(out["losses"]) == 7 and len(out["pretrain_losses"]) == 5 == ta.num_epochs
    # the explicit sequence
    eng, beh, rows, draw = tb._engine, tb._behavior_engine, len(replay), 2
    eng._ensure_bound(); beh._ensure_bound()
    var = N.QnetVariant(0, None, None, None, None, 1)
    pre, losses = [], []
    for _ in range(5):
        hp = tb.behavior_optimizer.hyper(tb.gamma, 1.0, 1.0 / B)
        if beh.can_sample:
            beh.learn_sampled(hp, *replay.arrays(), rows, B, SEED, draw, variant=var)
        else:
            beh.learn_indexed(hp, *replay.arrays(), E.sample_indices(rows, B, SEED, draw, device=DEV), variant=var)
        tb.behavior_optimizer.step_count = hp.step
        pre.append(beh.stats[2:3].clone())
        draw += 1
    for i in range(7):
        hp = tb.optimizer.hyper(tb.gamma, 0.0, 1.0 / B)
        if eng.can_sample:
            eng.bcq_learn_sampled(beh, hp, *replay.arrays(), rows, B, SEED, draw, tb.threshold)
        else:
            eng.bcq_learn_indexed(beh, hp, *replay.arrays(), E.sample_indices(rows, B, SEED, draw, device=DEV), tb.threshold)
        tb.optimizer.step_count = hp.step
        losses.append(eng.stats[:1].clone())
        draw += 1
        if i % 3 == 0:
            tb.sync_target()
    tb._draws = draw
    assert_state_equal(trainer_state(ta), trainer_state(tb))
    assert ta._draws == 14 and ta.optimizer.step_count == 7 and ta.behavior_optimizer.step_count == 5
    assert np.array_equal(out["losses"], torch.cat(losses).cpu().numpy()) and np.isfinite(out["losses"]).all()
    assert np.array_equal(out["pretrain_losses"], torch.cat(pre).cpu().numpy().astype(np.float64) + np.log(A))
    assert np.isfinite(out["pretrain_losses"]).all() and (out["pretrain_losses"] > 0).all()
    fresh = make_trainer("bcq", tmp_path, q_hidden=q_hidden)
    assert not torch.equal(fresh._engine.params, ta._engine.params)
    assert not torch.equal(fresh._behavior_engine.params, ta._behavior_engine.params)
    assert torch.equal(ta._engine.params, ta._engine.params_tgt)                # i = 6 is due a sync, and it is the last step
    # pretrain=0 skips the behaviour steps
    tc = make_trainer("bcq", tmp_path, q_hidden=q_hidden)
    out_c = tc.train_offline_device(replay, 1, seed=SEED, pretrain=0)
    assert len(out_c["pretrain_losses"]) == 0 and tc.behavior_optimizer.step_count == 0 and tc._draws == 1
    assert torch.equal(tc._behavior_engine.params, fresh._behavior_engine.params)


@pytest.mark.parametrize("kind,q_hidden", [("cql", (64, 64)), ("cql", (160, 64)), ("ddqn", (64, 64))])
def test_train_offline_device_plain_q_equals_learn_step_calls(kind, q_hidden, tmp_path):
    from porl_amd.train.vector_online import learn_step
    replay = filled_replay()
    ta, tb = make_trainer(kind, tmp_path, q_hidden=q_hidden), make_trainer(kind, tmp_path, q_hidden=q_hidden)
    out = ta.train_offline_device(replay, 8, seed=SEED)
    tb._engine._ensure_bound()
    losses = []
    for i in range(8):
        learn_step(tb, replay, SEED, i)
        losses.append(tb._engine.stats[:1].clone())
        if i % 3 == 0:
            tb.sync_target()
    tb._draws = 8
    assert_state_equal(trainer_state(ta), trainer_state(tb))
    assert np.array_equal(out["losses"], torch.cat(losses).cpu().numpy()) and np.isfinite(out["losses"]).all()
    assert out["learn_steps"] == 8 == ta.optimizer.step_count and len(out["pretrain_losses"]) == 0
    assert not torch.equal(make_trainer(kind, tmp_path, q_hidden=q_hidden)._engine.params, ta._engine.params)
    # a second call continues the first
    tc = make_trainer(kind, tmp_path, q_hidden=q_hidden)
    tc.train_offline_device(replay, 8, seed=SEED)
    ta.train_offline_device(replay, 2, seed=SEED)
    tc.train_offline_device(replay, 2, seed=SEED)
    assert ta._draws == 10 and torch.equal(ta._engine.params, tc._engine.params)


def test_train_offline_device_refusals(tmp_path):
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.train.vector_offline import train_offline_device
    replay = filled_replay()
    for kind, word in (("per", "train_vectorized_per"), ("c51", "train_vectorized_dist"), ("qr", "train_vectorized_dist"),
                       ("iqn", "train_vectorized_iqn")):
        t = make_trainer(kind, tmp_path)
        with pytest.raises(NotImplementedError, match=word):
            train_offline_device(t, replay, 2)
        assert not hasattr(t, "_draws")
    t = make_trainer("dqn", tmp_path)
    t._exchange = type("Exchange", (), dict(active=True, world_size=2))()
    with pytest.raises(NotImplementedError, match="gradient exchange"):
        t.train_offline_device(replay, 2)
    t = make_trainer("bcq", tmp_path)
    before = trainer_state(t)
    with pytest.raises(ValueError, match="DeviceReplay"):
        t.train_offline_device(DeviceReplay(600, 38, DEV), 2)
    with pytest.raises(ValueError, match="DeviceReplay"):
        t.train_offline_device(t.replay_buffer, 2)
    with pytest.raises(ValueError, match="larger sample"):
        t.train_offline_device(DeviceReplay(600, 22, DEV), 2)
    with pytest.raises(ValueError, match="negative"):
        t.train_offline_device(replay, -1)
    assert_state_equal(before, trainer_state(t))


# ---- score --------------------------------------------------------------------------------------------------------------------
def act_of(kind, t, n, constrained):
    """The act call of the trainer's own vectorised loop at epsilon 0, written out."""
    if kind == "iqn":
        eng = t._native_engine(batch=max(t.batch_size, n))
        return lambda sim, step: eng.act_rows(sim.obs, t.num_quantiles_n_policy, 0.0, SEED, step, env_offset=sim.env_offset)
    if kind in ("c51", "qr"):
        return lambda sim, step: t._engine.act_rows_dist(sim.obs, t._dist_head(), 0.0, SEED, step, env_offset=sim.env_offset)
    if kind == "bcq":
        return lambda sim, step: t.act_rows(sim.obs, 0.0, SEED, step, env_offset=sim.env_offset, constrained=constrained)
    return lambda sim, step: t._engine.act_rows(sim.obs, 0.0, SEED, step, env_offset=sim.env_offset)


def hand_evaluate(act, sim, episodes, episode_step):
    """evaluate_policy_batched's bookkeeping for the discrete task: the score summed in fp64 from the fp32 rewards, the
    step an episode ended at (the last permitted one when it did not), goal and hit read from the step that ended it."""
    n, left, t0, rows = sim.n_envs, episodes, 0, []
    while left > 0:
        take = min(n, left)
        sim.reset()
        score = torch.zeros(n, dtype=torch.float64, device=DEV)
        last = torch.full((n,), episode_step - 1, dtype=torch.int64, device=DEV)
        done, goal, hit = (torch.zeros(n, dtype=torch.bool, device=DEV) for _ in range(3))
        for k in range(episode_step):
            out = sim.step(act(sim, t0 + k))
            score += out.reward.double()                       # a finished robot idles: its later rewards are 0
            fin = (out.terminated | out.truncated) & ~done
            last = torch.where(fin, torch.full_like(last, k), last)
            goal |= fin & out.terminated & (out.reward == 200.0)
            hit |= fin & out.terminated & (out.reward == -200.0)
            done |= fin
        rows.append(torch.stack([(last + 1).double(), score, goal.double(), hit.double()], dim=1)[:take].cpu().numpy())
        left -= take
        t0 += episode_step
    return np.concatenate(rows)


@pytest.mark.parametrize("kind,constrained", [("dqn", True), ("c51", True), ("qr", True), ("iqn", True), ("bcq", True),
                                              ("bcq", False)])
def test_evaluate_discrete_equals_a_hand_loop(kind, constrained, tmp_path):
    from porl_amd.evaluate import evaluate_discrete
    n, episodes = 64, 100                                      # two rounds, the second counts 36 robots
    t = make_trainer(kind, tmp_path)
    if kind == "bcq":                                          # a behaviour policy with an opinion, from a few steps of data
        t.train_offline_device(filled_replay(), 3, seed=SEED)
    before = trainer_state(t)
    # the simulator's own limit is 40: a robot still running after 20 steps is a timeout that the tallies never saw
    res = evaluate_discrete(t, make_sim(n, auto_reset=False, episode_step=40), episodes, episode_step=EP_STEP, seed=SEED,
                            constrained=constrained)
    assert_state_equal(before, trainer_state(t))               # parameters, moments, epsilon, counters, replay: untouched
    want = hand_evaluate(act_of(kind, t, n, constrained), make_sim(n, auto_reset=False, episode_step=40), episodes, EP_STEP)
    assert res["episode_steps"].shape == (episodes,) and res["episode_steps"].dtype == np.int64
    assert np.array_equal(res["episode_steps"], want[:, 0].astype(np.int64))
    assert np.array_equal(res["episode_scores"], want[:, 1])                    # fp64, bit for bit
    assert np.array_equal(res["episode_goals"], want[:, 2] != 0) and np.array_equal(res["episode_hits"], want[:, 3] != 0)
    assert res["steps"] == want[:, 0].mean() and res["success"] == want[:, 2].mean() and res["hits"] == want[:, 3].mean()
    assert abs(res["score"] - want[:, 1].mean()) <= 1e-9 * max(1.0, abs(want[:, 1]).max())
    assert abs(res["timeouts"] + res["success"] + res["hits"] - 1.0) < 1e-12
    assert 1 <= res["episode_steps"].min() and res["episode_steps"].max() == EP_STEP and res["timeouts"] > 0
    # polling for "every robot has finished" changes nothing
    polled = evaluate_discrete(t, make_sim(n, auto_reset=False, episode_step=40), episodes, episode_step=EP_STEP, seed=SEED,
                               constrained=constrained, poll_every=5)
    for key in res:
        assert np.array_equal(polled[key], res[key]), key
    assert_state_equal(before, trainer_state(t))
    # episode_step=None is the simulator's limit: truncation ends the episodes, the same bookkeeping holds
    res20 = evaluate_discrete(t, make_sim(n, auto_reset=False), 40, seed=SEED, constrained=constrained)
    want20 = hand_evaluate(act_of(kind, t, n, constrained), make_sim(n, auto_reset=False), 40, EP_STEP)
    assert np.array_equal(res20["episode_steps"], want20[:, 0].astype(np.int64)) and np.array_equal(res20["episode_scores"], want20[:, 1])
    assert np.array_equal(res20["episode_goals"], want20[:, 2] != 0) and np.array_equal(res20["episode_hits"], want20[:, 3] != 0)


def test_evaluate_discrete_poll_ends_a_round_early(tmp_path):
    """A goal radius that holds every goal: all robots finish at their first step, the poll after step 5 ends the round."""
    from porl_amd.evaluate import evaluate_discrete
    t = make_trainer("dqn", tmp_path)
    kw = dict(auto_reset=False, goal_radius=5.0)
    sim = make_sim(64, **kw)
    polled = evaluate_discrete(t, sim, 70, poll_every=5)
    assert bool((sim.counters[:, 0] == 1).all())
    full = evaluate_discrete(t, make_sim(64, **kw), 70)
    for key in full:
        assert np.array_equal(polled[key], full[key]), key
    assert full["success"] == 1.0 and full["steps"] == 1.0 and full["score"] == 200.0 and full["timeouts"] == 0.0


def test_evaluate_discrete_refusals(tmp_path):
    from porl_amd.evaluate import evaluate_discrete
    t = make_trainer("dqn", tmp_path)
    with pytest.raises(ValueError, match="auto_reset"):
        evaluate_discrete(t, make_sim(), 4)
    with pytest.raises(ValueError, match="step limit"):
        evaluate_discrete(t, make_sim(auto_reset=False), 4, episode_step=21)
    with pytest.raises(ValueError, match="observes"):
        evaluate_discrete(t, make_sim(n_beams=36, auto_reset=False), 4)
    with pytest.raises(ValueError, match="positive"):
        evaluate_discrete(t, make_sim(auto_reset=False), 0)
