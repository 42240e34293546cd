"""The discrete lidar navigation task on the device (csrc/navsim_discrete.hpp, porl_amd/env/env.py) per element against
the fp64 numpy restatement tests/helpers/navdisc_cases.py; the replay target, porl_qnet_select, porl_qnet_act_rows and the
single-robot `Env`.

Tolerances.  Exact: flags, status, counters, the integer columns of the tallies, the +-200 rewards, and the heading and
distance entries of an observation — they are float32 of a two-decimal fp64 value, and the roll-out keeps 100 * heading,
100 * distance and 500 * tr further than 1e-7 from a half (tests/test_navdisc_host.py), so an ulp of fp64 cannot move
them.  Scan entries and shaped rewards: within 1 fp32 ulp — the two sides differ only in fp64 sincos, atan2 and exp2, by
an ulp of fp64, which can flip at most one fp32 rounding.  fp64 state: 1e-12.  Tally returns: T * 2**-23 * sum |r| per
robot (each of the T rewards summed may differ by its fp32 ulp).
"""
import contextlib
import io

import numpy as np
import pytest
import torch

from helpers import navdisc_cases as DC
from helpers import navsim_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ordinal(a):
    """float32 -> int64 that orders like the floats, so |ordinal(a) - ordinal(b)| counts the floats between them."""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def assert_ulp(got, want, what, ulps=1):
    got, want = np.atleast_1d(np.asarray(got, np.float32)), np.atleast_1d(np.asarray(want, np.float32))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not (np.isnan(got) | np.isnan(want)).any(), what
    d = np.abs(ordinal(got) - ordinal(want))
    print(f"{what}: max ulp distance {int(d.max()) if d.size else 0}, differing {int((d > 0).sum())} of {d.size}")
    assert d.max(initial=0) <= ulps, (what, int(d.max()), np.argwhere(d > ulps)[:5])


def device_sim(n, n_actions=5, **kw):
    from porl_amd.env import DiscreteLidarNavSim, NavWorld
    return DiscreteLidarNavSim(NavWorld.lattice(), n, n_actions=n_actions, **kw)


def hand_over(sim, oracle):
    """The device's state, read back and given to the restatement (not its tallies: those it keeps summing itself)."""
    oracle.state[:] = sim.state.cpu().numpy()
    oracle.counters[:] = sim.counters.cpu().numpy()
    oracle.obs[:] = sim.obs.cpu().numpy()


def assert_obs(got, want, nb, what):
    got, want = np.asarray(got), np.asarray(want)
    assert_ulp(got[:, :nb], want[:, :nb], what + " scan")
    assert np.array_equal(got[:, nb:], want[:, nb:]), (what, "heading / distance")


def compare_step(sim, oracle, actions, tag, replay=None):
    hand_over(sim, oracle)
    nb = oracle.p["n_beams"]
    want = oracle.step(actions)
    out = sim.step(torch.from_numpy(np.asarray(actions, np.int64)).to(DEV), replay=replay)
    flags = (out.terminated.int() | (out.truncated.int() << 1)).cpu().numpy()
    assert np.array_equal(flags, want["flags"]), tag
    assert np.array_equal(out.status.cpu().numpy(), want["status"]), tag
    r = out.reward.cpu().numpy()
    term = (want["flags"] & 1) != 0
    assert np.array_equal(r[term], want["reward"][term]) and (np.abs(r[term]) == 200).all(), tag
    assert_ulp(r[~term], want["reward"][~term], tag + " shaped reward")
    assert_obs(out.next_obs.cpu().numpy(), want["next_obs"], nb, tag + " next_obs")
    assert_obs(sim.obs.cpu().numpy(), oracle.obs, nb, tag + " obs")
    assert np.abs(sim.state.cpu().numpy() - oracle.state).max() <= 1e-12, tag
    assert np.array_equal(sim.counters.cpu().numpy(), oracle.counters), tag
    return out, want


@pytest.mark.parametrize("n_beams,n_actions,T", [(360, 5, DC.ROLLOUT["T"]), (37, 5, 5), (360, 3, 5)])
def test_steps_match_the_restatement_per_element(n_beams, n_actions, T):
    """N = 24 robots, episode_step = 25, seed 9, auto_reset, every third robot steering at the goal and the others on
    uniform indices from default_rng([seed, t]).  Each step starts from the device's own state, read back and handed to the
    restatement.  The 40-step roll-out meets 14 hits, 3 goals and 20 step limits (pinned on the host)."""
    cfg = DC.ROLLOUT
    p = DC.params(episode_step=cfg["episode_step"], n_beams=n_beams)
    sim = device_sim(cfg["n"], n_actions, seed=cfg["seed"], auto_reset=True, episode_step=cfg["episode_step"], n_beams=n_beams)
    oracle = DC.Sim(NC.lattice(), cfg["n"], n_actions, seed=cfg["seed"], auto_reset=True, p=p)
    oracle.reset()
    sim.reset()
    assert sim.obs.shape == (cfg["n"], n_beams + 2)
    assert_obs(sim.obs.cpu().numpy(), oracle.obs, n_beams, "reset obs")
    assert np.abs(sim.state.cpu().numpy() - oracle.state).max() <= 1e-12
    assert np.array_equal(sim.counters.cpu().numpy(), oracle.counters)
    abs_r = np.zeros(cfg["n"])
    ends = 0
    for t in range(T):
        a = DC.rollout_actions(sim.obs.cpu().numpy(), t, cfg["seed"], n_actions, n_beams, p)
        out, want = compare_step(sim, oracle, a, f"t={t}")
        abs_r += np.abs(want["reward"].astype(np.float64))
        ends += int((want["flags"] != 0).sum())
    geo, thr, rst, rnd = oracle.margins()
    print(f"episodes ended {ends}; margins: geometric {geo:.3e}, thresholds {thr:.3e}, reset {rst:.3e}, roundings {rnd:.3e}")
    assert min(geo, thr, rst) > NC.MARGIN and rnd > DC.MARGIN_ROUND          # on the states actually met
    tal = sim.tallies.cpu().numpy()
    assert np.array_equal(tal[:, [0, 2, 3]], oracle.tallies[:, [0, 2, 3]])
    assert tal[:, 0].sum() == ends and (ends >= 30 or T < 40)
    bound = T * 2.0 ** -23 * abs_r
    assert (np.abs(tal[:, 1] - oracle.tallies[:, 1]) <= bound).all(), (np.abs(tal[:, 1] - oracle.tallies[:, 1]).max(), bound.min())
    assert (np.abs(sim.returns.cpu().numpy() - oracle.returns) <= bound).all()
    assert not bool((sim.counters[:, 2] & 256).any())


def test_frozen_robots_and_clamped_indices():
    from porl_amd.buffer.device_replay import DeviceReplay
    n = 8
    sim = device_sim(n, seed=3, episode_step=3)
    oracle = DC.Sim(NC.lattice(), n, 5, seed=3, p=DC.params(episode_step=3))
    replay = DeviceReplay(32, sim.obs_dim, DEV)
    sim.reset()
    oracle.reset()
    raw = np.array([-3, 0, 4, 5, 99, 2, -(2 ** 40), 2 ** 40], np.int64)
    clamped = np.clip(raw, 0, 4)
    for t in range(3):
        out, want = compare_step(sim, oracle, raw, f"t={t}", replay=replay)
        assert np.array_equal(want["actions"], clamped)
        ran = want["ran"]
        got = replay.actions[t * n:(t + 1) * n].cpu().numpy()
        assert np.array_equal(got[ran], clamped[ran])                         # the clamped index is what the replay receives
    assert bool(((sim.counters[:, 2] & 0xff) != 0).all())                     # every robot reached the limit (or ended before)
    assert (sim.counters[:, 2].cpu().numpy() == NC.TIMELIMITED).all()         # (with this seed nobody ended before)
    # a further step changes nothing and writes nothing
    for arr in replay.arrays():
        arr[24:32] = -7
    before = [x.clone() for x in (sim.state, sim.counters, sim.obs, sim.tallies, sim.returns, *replay.arrays())]
    out = sim.step(torch.from_numpy(raw).to(DEV), replay=replay)
    for x, y in zip(before, (sim.state, sim.counters, sim.obs, sim.tallies, sim.returns, *replay.arrays())):
        assert torch.equal(x, y)
    assert not bool(out.reward.any()) and not bool(out.terminated.any()) and not bool(out.truncated.any())
    assert torch.equal(out.next_obs, sim.obs) and torch.equal(out.status.long(), sim.counters[:, 2])
    # reset(mask) wakes exactly the masked robot
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[5] = True
    sim.reset(mask)
    cn = sim.counters.cpu().numpy()
    assert cn[5].tolist()[:3] == [0, 2, 0]
    others = [i for i in range(n) if i != 5]
    assert np.array_equal(cn[others], before[1].cpu().numpy()[others])
    assert torch.equal(sim.state[others], before[0][others]) and torch.equal(sim.obs[others], before[2][others])
    assert not torch.equal(sim.state[5], before[0][5])
    out = sim.step(torch.full((n,), 2, dtype=torch.int64, device=DEV))
    assert out.status.cpu().numpy()[5] == 0 and int(sim.counters[5, 0]) == 1 and torch.equal(sim.state[others], before[0][others])


def test_replay_target_receives_each_transition():
    """Capacity 50, N = 24, three steps from bases 0, 24, 48: the third wraps.  Each array sits in front of a canary block."""
    from porl_amd.buffer.device_replay import DeviceReplay
    n, cap, FILL, CANARY = 24, 50, -7.0, 12345.0
    sim = device_sim(n, seed=5, auto_reset=True, episode_step=2)
    S = sim.obs_dim
    replay = DeviceReplay(cap, S, DEV)
    pad = 4096
    blocks = {}
    for name in ("states", "next_states", "actions", "rewards", "dones"):
        like = getattr(replay, name)
        big = torch.full((like.numel() + pad,), CANARY, dtype=torch.float64, device=DEV).to(like.dtype)
        big[:like.numel()] = FILL
        blocks[name] = big
        setattr(replay, name, big[:like.numel()].view(like.shape))
    sim.reset()
    rng = np.random.default_rng(0)
    held = {}
    for step, base in enumerate((0, 24, 48)):
        assert replay.position == base
        obs_before = sim.obs.clone()
        a = torch.from_numpy(rng.integers(-1, 7, n)).to(DEV)
        out = sim.step(a, replay=replay)
        slots = (base + torch.arange(n, device=DEV)) % cap
        done = (out.terminated | out.truncated).float()
        assert torch.equal(replay.states[slots], obs_before)
        assert torch.equal(replay.next_states[slots], out.next_obs)
        assert torch.equal(replay.actions[slots], a.clamp(0, 4))
        assert torch.equal(replay.rewards[slots].view(torch.int32), out.reward.view(torch.int32))      # bit for bit
        assert torch.equal(replay.dones[slots], done)
        if step == 0:
            held = {k: getattr(replay, k)[22:24].clone() for k in blocks}
        if step == 1:                                           # the 2 slots never addressed so far keep their fill value
            for k in blocks:
                assert bool((getattr(replay, k)[48:50] == FILL).all()), k
            assert bool(done.any())                              # episode_step = 2: the second step truncates
    assert replay.position == 22 and len(replay) == cap
    for k in blocks:                                            # the wrap stopped at slot 21; nothing ran past an array's end
        assert torch.equal(getattr(replay, k)[22:24], held[k]), k
        assert bool((blocks[k][getattr(replay, k).numel():] == CANARY).all()), k
    # a replay narrower than N, or of another row width, is refused
    with pytest.raises(ValueError, match="share a slot"):
        sim.step(torch.zeros(n, dtype=torch.int64, device=DEV), replay=DeviceReplay(23, S, DEV))
    with pytest.raises(ValueError, match="rows of"):
        sim.step(torch.zeros(n, dtype=torch.int64, device=DEV), replay=DeviceReplay(64, S + 1, DEV))
    with pytest.raises(ValueError, match="int64"):
        sim.step(torch.zeros(n, dtype=torch.int32, device=DEV))


# ---- select / act_rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 5])
def test_select_matches_the_restatement(A):
    from porl_amd.engine import qnet_select
    n = 130                                                     # beyond two waves, not a multiple of the block
    rng = np.random.default_rng(A)
    q = rng.standard_normal((n, A)).astype(np.float32)
    q[::7] = np.float32(0.5)                                    # rows of ties
    q[3, A - 1] = np.nan
    wide = torch.full((n, A + 3), 9e9, dtype=torch.float32, device=DEV)       # a row stride above the row width
    wide[:, :A] = torch.from_numpy(q).to(DEV)
    for eps in (0.0, 1.0, 0.3):
        for t in (0, 5):
            got = qnet_select(wide[:, :A], eps, 11, t, env_offset=2)
            assert got.dtype == torch.int64 and got.device.type == "cuda"
            assert np.array_equal(got.cpu().numpy(), DC.select(q, eps, 11, t, env_offset=2)), (eps, t)
    greedy = qnet_select(torch.from_numpy(q).to(DEV), 0.0, 11, 0)
    assert torch.equal(greedy, torch.argmax(torch.from_numpy(q).to(DEV), dim=1))
    assert int(greedy[3]) == A - 1 and int(greedy[0]) == 0      # the NaN is the maximum; a tie goes to the lowest index
    explore = qnet_select(wide[:, :A], 1.0, 11, 0).cpu().numpy()
    assert set(explore.tolist()) == set(range(A))
    # one run over 64 robots equals two runs over 32 with env_offset 0 and 32
    q64 = torch.from_numpy(q[:64].copy()).to(DEV)
    both = qnet_select(q64, 0.3, 4, 9)
    assert torch.equal(both[:32], qnet_select(q64[:32], 0.3, 4, 9, env_offset=0))
    assert torch.equal(both[32:], qnet_select(q64[32:], 0.3, 4, 9, env_offset=32))
    from porl_amd import _native as N
    with pytest.raises(N.NativeError, match="epsilon"):
        qnet_select(q64, 1.5, 4, 9)


@pytest.mark.parametrize("dueling", [False, True])
def test_act_rows_equals_forward_then_select(dueling, tmp_path):
    """N = 70 rows through an engine of max_batch 32: three chunks, the last partial.  engine.forward takes at most
    max_batch rows, so the reference walks the same chunks."""
    from porl_amd.engine import qnet_select
    from porl_amd.net.q_network import DuelingQNetwork, QNetwork
    from porl_amd.train.dddqn_trainer import DDDQNTrainer
    from porl_amd.train.dqn_trainer import DQNTrainer
    torch.manual_seed(1)
    kw = dict(device=DEV, batch_size=32, max_batch=32, log_dir=str(tmp_path))
    if dueling:
        t = DDDQNTrainer(38, 5, 0.99, network=lambda s, a: DuelingQNetwork(s, a, [64, 64]), **kw)
    else:
        t = DQNTrainer(38, 5, 0.99, network=lambda s, a: QNetwork(s, a, [64, 64]), **kw)
    eng = t._engine
    assert eng.cfg.max_batch == 32
    obs = torch.randn(70, 38, device=DEV)
    want_q = torch.cat([eng.forward(obs[r:r + 32]) for r in (0, 32, 64)])
    assert torch.equal(want_q, torch.cat([t.q_network(obs[r:r + 32]) for r in (0, 32, 64)]))
    for eps in (0.0, 0.4):
        q = torch.full((70, 5), float("nan"), device=DEV)
        got = eng.act_rows(obs, eps, 21, 6, env_offset=3, q=q)
        assert torch.equal(q, want_q)                           # bit for bit
        assert torch.equal(got, qnet_select(want_q, eps, 21, 6, env_offset=3))
    assert torch.equal(eng.act_rows(obs, 0.0, 0, 0), want_q.argmax(dim=1))
    tgt = eng.act_rows(obs[:5], 0.0, 0, 0, which=1)
    assert torch.equal(tgt, eng.forward(obs[:5], which=1).argmax(dim=1))


# ---- Env --------------------------------------------------------------------------------------------------------------------
def test_env_protocol_and_episodes(tmp_path):
    from porl_amd.env import Env
    env = Env(5, 362, rank_update_interval=2, seed=4)
    oracle = DC.Sim(NC.lattice(), 1, 5, seed=4, p=DC.PARAMS)
    assert (env.rank, env.cur_episode, env.status, env.action_size, env.namespace) == (0, 0, "initialized", 5, "tb3")
    rng = np.random.default_rng(2)
    for ep in range(3):
        state, info = env.reset()
        assert isinstance(state, np.ndarray) and state.shape == (362,) and state.dtype == np.float32
        assert info == {"status": "running"} and env.cur_episode == ep + 1 and env.cur_step == 0
        if ep == 2:                                             # the third episode is drawn in the square of rank 1
            first, oracle = oracle, DC.Sim(NC.lattice(rank=1), 1, 5, seed=4, p=DC.params(origin_x=-5.0, origin_y=5.0))
            oracle.counters[:] = first.counters
            assert min(first.margins()[:3]) > NC.MARGIN and first.margins()[3] > DC.MARGIN_ROUND
        oracle.reset()
        assert_obs(state[None], oracle.obs, 360, f"episode {ep} reset")
        for k in range(6):
            a = int(rng.integers(5))
            s2, r, done, trunc, info = env.step(a)
            assert isinstance(s2, np.ndarray) and s2.shape == (362,) and s2.dtype == np.float32
            assert type(r) is float and type(done) is bool and type(trunc) is bool and set(info) == {"status"}
            assert env.cur_step == k + 1
            want = oracle.step([a])
            assert_obs(s2[None], want["next_obs"], 360, f"episode {ep} step {k}")
            assert_ulp(np.float32(r), want["reward"][0], "reward")
            assert (done, trunc) == (bool(want["flags"][0] & 1), bool(want["flags"][0] & 2))
            assert info["status"] == NC_STATUS[int(want["status"][0])]
            if done or trunc:
                break
    # rank advances after rank_update_interval = 2 resets, and the spawn square moves with it (lattice(1): x in [-5, 0])
    assert env.rank == 1 and env.cur_episode == 3
    x, y = env.sim.state[0, :2].tolist()
    assert -5.0 < x < 0.0 and 5.0 < y < 10.0
    assert int(env.sim.counters[0, 1]) == 3                     # the episode number went on counting
    env.render()
    env.close()
    geo, thr, rst, rnd = oracle.margins()
    assert min(geo, thr, rst) > NC.MARGIN and rnd > DC.MARGIN_ROUND


NC_STATUS = ("running", "hit", "goal", "timelimited")


def test_train_online_runs_in_the_env(tmp_path):
    from porl_amd.env import Env
    from porl_amd.train.dqn_trainer import DQNTrainer
    torch.manual_seed(0)
    t = DQNTrainer(362, 5, 0.99, device=DEV, log_dir=str(tmp_path))
    env = Env(5, 362, seed=1)
    np.random.seed(0)                      # epsilon = 1: these indices end no episode within 5 steps (restatement, host)
    with contextlib.redirect_stdout(io.StringIO()):
        rewards = t.train_online(env, num_episodes=2, max_steps=5)
    assert len(rewards) == 2 and all(np.isfinite(rewards))
    assert len(t.replay_buffer) == 10 and env.cur_episode == 2
    assert np.array_equal(t.replay_buffer.next_states[:4], t.replay_buffer.states[1:5])       # one episode's chain
    assert set(np.unique(t.replay_buffer.actions[:10])) <= set(range(5))
