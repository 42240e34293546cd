"""The lidar navigation simulator on the device (csrc/navsim.hpp, porl_amd/env) per element against the fp64 numpy
restatement tests/helpers/navsim_cases.py and the recorded reset draws tests/golden/navsim_reset.npz.

Tolerances: a range, an observation entry and a reward are within 1 fp32 ulp of float32(oracle) — the kernel and the
restatement differ only in fp64 sin / cos / atan2, ~1e-16 relative, which can flip one fp32 rounding at most; the
rewards +-500, `no_return` entries, flags, status and counters are exact; the fp64 state agrees to 1e-12.  Every case keeps
each discontinuous decision further than NC.MARGIN = 1e-9 from its tie, asserted on the states the test actually meets.
"""
import math

import numpy as np
import pytest
import torch

import porl_amd.ops  # noqa: F401  (registers torch.ops.porl_hip.*)
from conftest import load_golden
from helpers import navsim_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ordinal(a):
    """float32 -> int64 that orders like the floats, so |ordinal(a) - ordinal(b)| counts the floats between them."""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def assert_ulp(got, want, what, ulps=1):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    both_nan = np.isnan(got) & np.isnan(want)
    d = np.where(both_nan, 0, np.abs(ordinal(got) - ordinal(want)))
    assert not (np.isnan(got) ^ np.isnan(want)).any(), what
    print(f"{what}: max ulp distance {int(d.max()) if d.size else 0}, differing {int((d > 0).sum())} of {d.size}")
    assert d.max(initial=0) <= ulps, (what, int(d.max()), np.argwhere(d > ulps)[:5])


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


def world_of(w):
    from porl_amd.env import NavWorld
    return NavWorld(w[0], w[1], origin=(NC.PARAMS["origin_x"], NC.PARAMS["origin_y"])).to(DEV)


def device_sim(n=NC.ROLLOUT["n"], world=None, **kw):
    from porl_amd.env import LidarNavSim
    return LidarNavSim(world_of(NC.lattice() if world is None else world), n, **kw)


# ---- scan -----------------------------------------------------------------------------------------------------------------
WORLDS = {"lattice": (NC.lattice, NC.lattice_poses), "oblique": (NC.oblique, NC.oblique_poses)}


@pytest.mark.parametrize("n_beams", [360, 130, 37])
@pytest.mark.parametrize("kind", ["lattice", "oblique"])
def test_scan_matches_the_oracle_per_range(kind, n_beams):
    from porl_amd.env import nav_scan
    p = NC.params(n_beams=n_beams)
    world, poses = WORLDS[kind][0](), WORLDS[kind][1](96, 7 + n_beams, p)
    margin = NC.margins(world, poses, p)
    print(f"{kind} n_beams={n_beams}: smallest margin {margin:.3e}")
    assert margin > NC.MARGIN
    want = NC.cast(world[0], world[1], poses, p)
    w = world_of(world)
    got = nav_scan(w.segments, w.circles, t64(poses), n_beams=n_beams).cpu().numpy()
    miss = want == np.float32(10.0)
    assert miss.any() and (~miss).any()
    assert np.array_equal(got == np.float32(10.0), miss)                           # no_return entries are exact
    assert_ulp(got, want, f"scan {kind} {n_beams}")


def test_scan_with_nothing_in_range_and_a_strided_out():
    from porl_amd.env import nav_scan
    far = (np.array([[50, -1, 50, 1]], np.float32), np.zeros((0, 3), np.float32))
    w = world_of(far)
    got = nav_scan(w.segments, w.circles, t64([[0.0, 0.0, 0.3]]))
    assert got.shape == (1, 360) and bool((got == 10.0).all())
    # a strided out: columns 3..362 of a wider buffer, whose other columns stay as they were
    world, poses = NC.lattice(), NC.lattice_poses(5, 99)
    buf = torch.full((5, 400), -7.0, device=DEV)
    w = world_of(world)
    nav_scan(w.segments, w.circles, t64(poses), out=buf[:, 3:363])
    host = buf.cpu().numpy()
    assert (host[:, :3] == -7).all() and (host[:, 363:] == -7).all()
    assert_ulp(host[:, 3:363], NC.cast(world[0], world[1], poses), "strided scan")
    # closed form on the device: a wall at distance D straight ahead reads D / cos(angle)
    wall = (np.array([[2, -50, 2, 50]], np.float32), np.zeros((0, 3), np.float32))
    w = world_of(wall)
    r = nav_scan(w.segments, w.circles, t64([[0.0, 0.0, 0.0]]))[0].cpu().numpy().astype(np.float64)
    for i in (0, 10, 45, 315):
        assert abs(r[i] - 2.0 / math.cos(math.radians(i))) < 4e-7
    assert r[90] == 10.0 and r[180] == 10.0
    # the registered operator is the same call
    w = world_of(world)
    assert torch.equal(torch.ops.porl_hip.nav_scan(w.segments, w.circles, t64(poses), 130),
                       nav_scan(w.segments, w.circles, t64(poses), n_beams=130))


# ---- step: per element from identical state --------------------------------------------------------------------------------
def load_oracle(oracle, sim):
    oracle.state = sim.state.cpu().numpy().copy()
    oracle.counters = sim.counters.cpu().numpy().copy()
    oracle.obs = sim.obs.cpu().numpy().copy()


def compare_step(sim, oracle, actions, rows=False, tag=""):
    """One device step and one oracle step from the device's state; every output and the new state compared."""
    load_oracle(oracle, sim)
    n, W = sim.n_envs, sim.row_width
    store = torch.zeros(n, W + 3, device=DEV) if rows else None
    out = sim.step(torch.from_numpy(actions).to(DEV), rows=None if store is None else store[:, :W])
    want = oracle.step(actions, want_rows=rows)
    flags = (out.terminated.int() + 2 * out.truncated.int()).cpu().numpy()
    assert np.array_equal(flags, want["flags"]), tag
    assert np.array_equal(out.status.cpu().numpy(), want["status"]), tag
    assert np.array_equal(sim.counters.cpu().numpy(), oracle.counters), tag
    r, wr = out.reward.cpu().numpy(), want["reward"]
    big = np.abs(wr) == 500
    assert np.array_equal(r[big], wr[big]), tag
    assert_ulp(r, wr, f"{tag} reward")
    assert_ulp(out.next_obs.cpu().numpy(), want["next_obs"], f"{tag} next_obs")
    assert_ulp(sim.obs.cpu().numpy(), oracle.obs, f"{tag} obs")
    ds = np.abs(sim.state.cpu().numpy() - oracle.state).max()
    assert ds <= 1e-12, (tag, ds)
    if rows:
        assert_ulp(store[:, :W].cpu().numpy(), want["rows"], f"{tag} rows")
        assert bool((store[:, W:] == 0).all())
    return out


def test_rollout_steps_match_the_oracle_per_element():
    """N = 64 robots, T = 60 steps, episode_step = 40, seed 12345, every third robot steering at the goal and the others on
    collect.py:38's random command.  Each step starts from the device's own state, read back and handed to the oracle.
    With this file's command stream (numpy default_rng keyed by seed and step) the roll-out meets 37 hits, 7 goals and 46
    step limits, smallest geometric margin 1.2e-8, smallest threshold margin 3.1e-6 (tests/test_navsim_host.py pins the
    counts on the host); on the device every compared fp32 element came out bit-equal to float32(oracle)."""
    cfg = NC.ROLLOUT
    p = NC.params(episode_step=cfg["episode_step"])
    sim = device_sim(seed=cfg["seed"], auto_reset=True, episode_step=cfg["episode_step"])
    oracle = NC.Sim(NC.lattice(), cfg["n"], seed=cfg["seed"], auto_reset=True, p=p)
    oracle.reset()
    sim.reset()
    assert_ulp(sim.obs.cpu().numpy(), oracle.obs, "reset obs")
    assert np.abs(sim.state.cpu().numpy() - oracle.state).max() <= 1e-12
    assert np.array_equal(sim.counters.cpu().numpy(), oracle.counters)
    seen = {NC.HIT: 0, NC.GOAL: 0, NC.TIMELIMITED: 0}
    for t in range(cfg["T"]):
        a = NC.rollout_commands(sim.obs.cpu().numpy(), t)
        out = compare_step(sim, oracle, a, rows=(t % 7 == 0), tag=f"t={t}")
        st = out.status.cpu().numpy()
        for k in seen:
            seen[k] += int((st == k).sum())
    geo, thr, rst = oracle.margins()
    print(f"outcomes {seen}; margins: geometric {geo:.3e}, thresholds {thr:.3e}, reset {rst:.3e}; "
          f"smallest spawn range {oracle.min_spawn_scan:.4f}")
    assert min(geo, thr, rst) > NC.MARGIN                                   # on the states actually met
    assert all(v > 0 for v in seen.values()), seen                          # all three outcomes occur
    assert not bool((sim.counters[:, 2] & 256).any())                       # no reset ran into the draw cap
    assert oracle.min_spawn_scan >= 0.13


# ---- reset ------------------------------------------------------------------------------------------------------------------
def test_reset_matches_the_recorded_draws():
    z, _ = load_golden("navsim_reset")
    seeds, envs, eps = z["seed"], z["env"], z["episode"]
    checked = 0
    for seed in np.unique(seeds):
        for base in np.unique(envs // 1000 * 1000):
            sel = (seeds == seed) & (envs // 1000 * 1000 == base)
            n = int(envs[sel].max() - base) + 1
            sim = device_sim(n=n, seed=int(seed), env_offset=int(base))
            for e in np.unique(eps[sel]):
                c = torch.zeros(n, 4, dtype=torch.int64)
                c[:, 1] = int(e) - 1
                sim.set_state(counters=c)
                sim.reset()
                st, cn = sim.state.cpu().numpy(), sim.counters.cpu().numpy()
                for k in np.flatnonzero(sel & (eps == e)):
                    i = int(envs[k] - base)
                    assert np.abs(st[i, [0, 1, 3, 4]] - z["xy"][k]).max() <= 1e-12, (seed, envs[k], e)
                    assert cn[i].tolist() == [0, int(e), 0, int(z["draws"][k])]
                    assert st[i, 2] == 0.0
                    checked += 1
    assert checked == len(seeds) == 256


def test_reset_mask_touches_only_masked_robots():
    sim = device_sim(n=16, seed=5)
    sim.reset()
    before = (sim.state.clone(), sim.counters.clone(), sim.obs.clone())
    mask = torch.zeros(16, dtype=torch.bool, device=DEV)
    mask[[1, 6, 15]] = True
    obs = sim.reset(mask)
    assert obs is sim.obs
    keep = ~mask
    for b, a in zip(before, (sim.state, sim.counters, sim.obs)):
        assert torch.equal(b[keep], a[keep])
    assert sim.counters[mask][:, 1].tolist() == [2, 2, 2]
    assert not torch.equal(before[0][mask][:, :2], sim.state[mask][:, :2])


# ---- other behaviours -------------------------------------------------------------------------------------------------------
def test_finished_robot_is_frozen_and_clipped_commands():
    p = NC.params(episode_step=3)
    sim = device_sim(n=8, seed=11, episode_step=3)
    oracle = NC.Sim(NC.lattice(), 8, seed=11, p=p)
    sim.reset()
    a = np.array([[0.5, 3.0], [-0.2, -9.0], [np.nan, 0.3], [0.1, np.inf], [0.15, 1.5], [0.0, 0.0], [np.inf, -np.inf],
                  [0.07, 1e-5]], np.float32)
    W = sim.row_width
    for t in range(3):
        out = compare_step(sim, oracle, a, rows=True, tag=f"clip t={t}")
    final = out.status.tolist()                       # the step limit ends all of them; one may also have hit a pillar
    assert bool(out.truncated.all()) and all(v in (NC.HIT, NC.TIMELIMITED) for v in final) and final[2] == NC.TIMELIMITED
    # the clipped command is what the row holds
    rows = torch.zeros(8, W, device=DEV)
    frozen = (sim.state.clone(), sim.counters.clone(), sim.obs.clone())
    out = sim.step(torch.from_numpy(a).to(DEV), rows=rows)
    assert bool(torch.isnan(rows).all())
    assert out.reward.tolist() == [0.0] * 8 and not bool(out.terminated.any()) and not bool(out.truncated.any())
    assert out.status.tolist() == final
    assert torch.equal(out.next_obs, sim.obs)
    for b, c in zip(frozen, (sim.state, sim.counters, sim.obs)):
        assert torch.equal(b, c)
    # reset(mask) wakes one of them
    mask = torch.zeros(8, dtype=torch.bool, device=DEV)
    mask[2] = True
    sim.reset(mask)
    out = sim.step(torch.from_numpy(a).to(DEV))
    assert out.status.tolist() == final[:2] + [0] + final[3:] and sim.counters[2].tolist()[:2] == [1, 2]


def test_clipped_command_lands_in_the_row():
    sim = device_sim(n=4, seed=2)
    sim.reset()
    rows = torch.zeros(4, sim.row_width, device=DEV)
    a = torch.tensor([[0.5, 3.0], [-0.2, -9.0], [float("nan"), 0.3], [0.1, float("inf")]], device=DEV)
    sim.step(a, rows=rows)
    want = np.array([[0.15, 1.5], [0.0, -1.5], [0.0, 0.3], [0.1, 0.0]], np.float64).astype(np.float32)
    assert np.array_equal(rows[:, -2:].cpu().numpy(), want)


def test_pose_layout_rows_feed_the_episode_table_and_the_labels():
    """An env-major strided store: collect() writes robot i's trajectory contiguously; the episode table built from its
    flags equals the simulator's episode counters, and the A* labels of the 734-wide rows equal the restatement's."""
    from helpers import astar_cases as AC
    from porl_amd.dataloader.astar import astar_values, label_rows
    from porl_amd.dataloader.episodes import EpisodeIndex
    from porl_amd.env import collect
    n, T = 12, 45
    p = NC.params(episode_step=20)
    sim = device_sim(n=n, seed=77, layout="pose", auto_reset=True, episode_step=20)
    oracle = NC.Sim(NC.lattice(), n, seed=77, layout="pose", auto_reset=True, p=p)
    sim.reset()
    for t in range(3):                                                            # the pose layout, per element
        compare_step(sim, oracle, NC.rollout_commands(np.zeros((n, 362), np.float32), t), rows=True, tag=f"pose t={t}")
    sim.reset()
    first = sim.counters[:, 1].clone()
    gen = torch.Generator(device=DEV).manual_seed(3)
    rows, timeouts = collect(sim, None, T, generator=gen)
    assert rows.shape == (n * T, 734) and timeouts.shape == (n * T,)
    host, S = rows.cpu().numpy(), 365
    assert not np.isnan(host).any()
    # a trajectory is contiguous: s' of a step is s of the robot's next step unless an episode ended
    assert timeouts.dtype == torch.float32
    ended = timeouts.cpu().numpy() != 0
    for i in range(n):
        for t in range(T - 1):
            k = i * T + t
            if not ended[k]:
                assert np.array_equal(host[k, S + 1:2 * S + 1], host[k + 1, :S])
    idx = EpisodeIndex.from_replay(rows, timeouts=timeouts)
    assert idx.trailing == 0
    done_last = (sim.counters[:, 0] == 0).cpu().numpy()                           # the last step closed an episode
    per_robot = (sim.counters[:, 1] - first).cpu().numpy() + 1 - done_last
    assert int(idx.starts.shape[0]) == int(per_robot.sum())
    ends = idx.ends.cpu().numpy()
    assert all(((ends >= i * T) & (ends < (i + 1) * T)).sum() == per_robot[i] for i in range(n))
    assert set(range(T - 1, n * T, T)) <= set(ends.tolist())                      # no episode joins two robots
    # the labels: the device pass on collected rows against the numpy restatement on the same rows (those whose every
    # comparison in the labelling pass is away from a tie, as tests/test_astar_gpu.py chooses its rows)
    pick = [k for k in range(0, n * T, 5) if AC.margins_ok(host[k])]
    assert len(pick) >= 40, len(pick)
    sub = rows[pick].contiguous()
    st_w, len_w, val_w = AC.label_all(host[pick])
    value, path_len, status = (x.cpu().numpy() for x in astar_values(sub))
    keep = st_w == 0
    assert np.array_equal(status, st_w) and keep.sum() >= 20
    assert np.array_equal(path_len[keep], len_w[keep]) and np.array_equal(value[keep], val_w[keep])
    want = np.concatenate([host[pick][keep][:, :360], val_w[keep][:, None]], axis=1)
    assert np.array_equal(label_rows(sub).cpu().numpy(), want)


# ---- determinism ------------------------------------------------------------------------------------------------------------
def _roll(sim, T, lo=0, n_total=None):
    sim.reset()
    outs = []
    for t in range(T):
        n_total = n_total or sim.n_envs
        u = np.random.default_rng([4, t]).random((n_total, 2))[lo:lo + sim.n_envs]
        a = torch.from_numpy(((u * 2 + [0, -1]) * [0.075, 1.5]).astype(np.float32)).to(DEV)
        o = sim.step(a)
        outs.append(torch.cat([o.next_obs, o.reward[:, None], o.status[:, None].float(), sim.obs], dim=1))
    return torch.stack(outs), sim.state.clone(), sim.counters.clone()


def test_rollouts_are_deterministic_and_split_by_env_offset():
    kw = dict(seed=9, auto_reset=True, episode_step=10)
    a = _roll(device_sim(n=64, **kw), 25)
    b = _roll(device_sim(n=64, **kw), 25)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    lo = _roll(device_sim(n=32, env_offset=0, **kw), 25, 0, 64)
    hi = _roll(device_sim(n=32, env_offset=32, **kw), 25, 32, 64)
    assert torch.equal(a[0], torch.cat([lo[0], hi[0]], dim=1))
    assert torch.equal(a[1], torch.cat([lo[1], hi[1]])) and torch.equal(a[2], torch.cat([lo[2], hi[2]]))


# ---- wrappers ---------------------------------------------------------------------------------------------------------------
class SteeringAgent:
    """select_action for test.py's loop: the normalised action whose command is NC.steer's."""

    def select_action(self, state):
        return NC.steer_normalised(state.cpu().numpy())


def _args(**kw):
    from types import SimpleNamespace
    return SimpleNamespace(namespace="tb3", state_size=362, action_size=2, device=DEV, **kw)


def test_env_and_evaluate_policy_follow_the_oracle():
    import statistics
    from porl_amd.env.gazebo import Env
    from porl_amd.evaluate import evaluate_policy, evaluate_policy_batched
    env = Env("tb3", 362, 2, seed=21, episode_step=500)
    state, info = env.reset()
    assert state.shape == (362,) and state.dtype == np.float32 and info == {"status": "running"}
    s2, r, term, trunc, info = env.step(np.array([0.1, 0.2]))
    assert s2.shape == (362,) and isinstance(r, float) and term is False and trunc is False and info["status"] == "running"
    # the roll-out loop of test.py, three episodes of one robot: episodes 1, 2, 3 of stream (seed 21, env 0)
    E, T = 3, 60
    env = Env("tb3", 362, 2, seed=21)
    got = evaluate_policy(SteeringAgent(), _args(test_episodes=E, episode_step=T), env=env)
    o = NC.Sim(NC.lattice(), 1, seed=21, p=NC.params())
    ts, scores, succ, mass = [], [], [], 0.0
    for e in range(E):
        o.reset()
        score = 0.0
        for t in range(T):
            cmd = NC.steer(o.obs)
            out = o.step(cmd)
            score += float(out["reward"][0])
            mass += abs(float(out["reward"][0]))
            if out["flags"][0] & 1 or t == T - 1:
                ts.append(t), scores.append(score), succ.append(float(o.counters[0, 2] == NC.GOAL))
                break
    print("evaluate_policy", got, (ts, scores, succ), o.margins())
    assert min(o.margins()) > NC.MARGIN
    assert got[0] == statistics.fmean(ts) and got[2] == statistics.fmean(succ)
    # each reward is an fp32 value within 1 ulp (2^-23 relative) of the oracle's from the same state, and the free-running
    # fp64 states stay within 1e-12 of each other, which moves a reward by at most ~1e-11; both sides sum in a Python float
    bound = (mass * 2.0 ** -23 + E * T * 1e-11) / E
    print(f"evaluate_policy score difference {abs(got[1] - statistics.fmean(scores)):.3e}, bound {bound:.3e}")
    assert abs(got[1] - statistics.fmean(scores)) <= bound
    assert sum(succ) >= 1                                                     # the steering agent does reach goals
    # batched: 8 robots, one episode each = the per-robot loops of Env(rank=i)
    from porl_amd.env import LidarNavSim, NavWorld
    sim = LidarNavSim(NavWorld.lattice(), 8, seed=21)
    act = lambda obs: torch.from_numpy(NC.steer(obs.cpu().numpy())).to(DEV)
    batched = evaluate_policy_batched(act, sim, 8, T)
    singles = [evaluate_policy(SteeringAgent(), _args(test_episodes=1, episode_step=T),
                               env=Env("tb3", 362, 2, rank=0, seed=21, world=NavWorld.lattice())
                               if i == 0 else _offset_env(i)) for i in range(8)]
    assert batched[0] == statistics.fmean(s[0] for s in singles)
    assert batched[2] == statistics.fmean(s[2] for s in singles)
    assert abs(batched[1] - statistics.fmean(s[1] for s in singles)) <= 1e-9 * max(1.0, abs(batched[1]))
    # the roll-out may not outlast the simulator's own step limit, and a command outside the robot's limits is an error
    with pytest.raises(ValueError, match="step limit"):
        evaluate_policy_batched(act, LidarNavSim(NavWorld.lattice(), 2, episode_step=5), 2, 6)
    with pytest.raises(ValueError, match="step limit"):
        evaluate_policy(SteeringAgent(), _args(test_episodes=1, episode_step=501), env=env)

    class TooFast:
        def select_action(self, state):
            return np.array([[1.5, 0.0]], np.float32)
    with pytest.raises(AssertionError, match="m/s"):
        evaluate_policy(TooFast(), _args(test_episodes=1, episode_step=3), env=env)


def _offset_env(i):
    """Env whose robot draws from stream (seed 21, env i) in the rank-0 world."""
    from porl_amd.env import LidarNavSim, NavWorld
    from porl_amd.env.gazebo import Env
    env = Env("tb3", 362, 2, rank=0, seed=21)
    env.sim = LidarNavSim(NavWorld.lattice(), 1, seed=21, env_offset=i)
    return env


def test_evaluate_policy_runs_real_agents():
    from types import SimpleNamespace
    from porl_amd.agent import GoalConditionedBC
    from porl_amd.agent.por import POR
    from porl_amd.agent.sorl import SORL
    from porl_amd.env import LidarNavSim, NavWorld
    from porl_amd.evaluate import evaluate_policy, evaluate_policy_batched, por_act, sorl_act
    torch.manual_seed(0)
    args = SimpleNamespace(state_size=362, hidden_dim=64, n_hidden=2, layer_norm=False, action_size=2, namespace="tb3",
                           device=DEV, test_episodes=2, episode_step=6)
    sorl = SORL(args, 100, 0.9, 10.0, device=DEV)
    por = POR(args, 100, 0.9, 10.0, device=DEV)
    por.set_execute_policy(GoalConditionedBC(362, 362, 2, 100, hidden_dim=64, bounded=True, device=DEV))
    sim = LidarNavSim(NavWorld.lattice(), 16, seed=1)
    for agent, act in ((sorl, sorl_act(sorl)), (por, por_act(por))):
        for triple in (evaluate_policy(agent, args), evaluate_policy_batched(act, sim, 20, 6)):
            assert len(triple) == 3 and all(math.isfinite(v) for v in triple), triple
            assert 0 <= triple[0] <= 5 and 0 <= triple[2] <= 1
