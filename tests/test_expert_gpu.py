"""The A* expert on the device (csrc/expert.hpp, porl_amd/env/expert.py) against the fp64 numpy restatement
tests/helpers/expert_cases.py and the reference planner's recorded paths tests/golden/expert_paths.npz.

Exact: every bit of a bitmap's interior, every cell of every cached field (integer pairs), every path cell, path_len,
status, tags.  Waypoints are cell centres (a product and a sum, no fma) or the goal as stored: exact too.  Commands and
scores are fp32 roundings of fp64 values that differ from the restatement's only through atan2 and cos (an ulp of fp64
each): within 1 fp32 ulp.  Where the roll-out meets a heading error that is itself rounding noise (a robot driving
straight at its waypoint: e ~ 1e-16) an ulp of the fp32 result is smaller than the fp64 libraries' absolute error, so
`assert_steer` also accepts |got - want| <= 1e-13: atan2 is good to an ulp of pi (4.4e-16) on either side, e is their
difference with yaw, and the largest factor applied to e is 1 / dt = 5.  Every case keeps each discontinuous decision
further than EC.MARGIN = 1e-9 from its tie, asserted on the states the test actually meets.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import expert_cases as EC
from helpers import navsim_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
ORIGIN = (NC.PARAMS["origin_x"], NC.PARAMS["origin_y"])


def ordinal(a):
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def assert_steer(got, want64, what):
    got = np.asarray(got, np.float32)
    want = np.asarray(want64, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(ordinal(got) - ordinal(want.astype(np.float32)))
    near = np.abs(got.astype(np.float64) - want) <= 1e-13
    print(f"{what}: max ulp distance {int(d.max())}, differing {int((d > 0).sum())} of {d.size}, "
          f"{int(((d > 1) & near).sum())} accepted by the absolute bound")
    assert ((d <= 1) | near).all(), (what, int(d.max()), np.argwhere((d > 1) & ~near)[:5])


def world_of(w, origin=ORIGIN):
    from porl_amd.env import NavWorld
    return NavWorld(w[0], w[1], origin=origin).to(DEV)


def sim_with(world, states, discrete=False, **kw):
    from porl_amd.env import DiscreteLidarNavSim, LidarNavSim
    sim = (DiscreteLidarNavSim if discrete else LidarNavSim)(world, len(states), **kw)
    sim.set_state(state=states)
    return sim


def host(t):
    return t.cpu().numpy()


def raw_field(fld, g):
    """The padded device row of a restated (w, h) field."""
    pad = np.full((g.h + 2, g.pw), EC.UNREACHED, np.uint32)
    pad[1:-1, 1:-1] = fld.T
    return pad.reshape(-1)


def device_rows(expert):
    return host(expert.fields).view(np.uint32)


# ---- rasterise ------------------------------------------------------------------------------------------------------------
RASTER = {"lattice": (EC.lattice_world, EC.lattice_grid), "oblique": (NC.oblique, EC.oblique_grid),
          "oblique_odd": (NC.oblique, EC.oblique_odd_grid), "tiny": (EC.tiny_world, EC.tiny_grid)}


@pytest.mark.parametrize("kind", list(RASTER))
def test_bitmap_matches_the_restatement_bit_for_bit(kind):
    from porl_amd.env import PlanGrid
    world, g = RASTER[kind][0](), RASTER[kind][1]()
    want, margin = EC.rasterize(world[0], world[1], g)
    print(f"{kind}: {g.w} x {g.h}, {g.pcells} padded cells, {int(want.sum())} blocked, smallest margin {margin:.3e}")
    assert margin > EC.MARGIN and want.any() and not want.all()
    if kind in ("lattice", "oblique_odd"):                     # (the 70 x 66 grid pads to 72 * 68 = 153 whole words)
        assert g.pcells % 32 and g.pcells % 64
    if kind == "tiny":
        assert g.pcells < 256 and g.pcells % 64                # fewer cells than threads; the last ballot straddles the end
    grid = PlanGrid(world_of(world), **g.kwargs())
    assert (grid.w, grid.h, grid.pcells) == (g.w, g.h, g.pcells)
    words = host(grid.bitmap).view(np.uint32)
    assert len(words) == (g.pcells + 31) // 32
    assert np.array_equal(EC.unpack_interior(words, g), want)
    occ = grid.occupancy()
    assert occ.shape == (g.w, g.h) and occ.dtype == torch.bool and np.array_equal(host(occ), want)
    if kind == "lattice":                                      # the defaults are this grid
        dflt = PlanGrid(world_of(world))
        assert (dflt.w, dflt.h, dflt.min_x, dflt.min_y, dflt.resolution, dflt.inflate) == (51, 51, *ORIGIN, 0.1, 0.18)
        assert torch.equal(dflt.bitmap, grid.bitmap)


# ---- field ----------------------------------------------------------------------------------------------------------------
def test_fields_match_the_restatement_cell_for_cell():
    from porl_amd.env import AStarExpert
    world, g = EC.room_world(), EC.lattice_grid()
    occ, margin = EC.rasterize(world[0], world[1], g)
    states = EC.field_states()
    sim = sim_with(world_of(world), states)
    ex = AStarExpert(sim)
    ex.fields.fill_(0x5A5A5A5A)
    before = ex.fields.clone()
    plan = ex.plan()
    pl = EC.Planner(g, occ)
    rows, tags = device_rows(ex), host(ex.tags)
    valid = []
    for i, st in enumerate(states):
        status, goal = pl.goal_cell(st)
        if status != EC.OK:                                    # blocked, off the grid, non-finite: nothing is touched
            assert tags[i] == 0 and torch.equal(ex.fields[i], before[i]), i
            continue
        valid.append(i)
        want = pl.field_of(goal)
        assert tags[i] == goal[1] * g.w + goal[0] + 1, i
        assert np.array_equal(rows[i], raw_field(want, g)), i
        a, b = ex.field(i)
        wa, wb = EC.pairs(want)
        assert a.dtype == torch.int32 and np.array_equal(host(a), wa) and np.array_equal(host(b), wb), i
    assert valid == [0, 1, 2, 3, 7] and min(margin, pl.margin) > EC.MARGIN
    # the sealed room's field reaches its nine cells only; the goal next to the wall reaches the whole room outside it
    assert int((host(ex.field(2)[0]) >= 0).sum()) == 9 and int((host(ex.field(1)[0]) >= 0).sum()) == int((~occ).sum()) - 9
    assert host(plan.status).tolist() == EC.STATUS_WANT[:8]
    # a second call: every tag names its goal cell, so nothing is relaxed and nothing changes
    again, tags2 = ex.fields.clone(), ex.tags.clone()
    ex.plan()
    assert torch.equal(ex.fields, again) and torch.equal(ex.tags, tags2)
    ex.invalidate()
    ex.plan()
    assert torch.equal(ex.fields, again) and torch.equal(ex.tags, tags2)


def test_fields_on_the_smallest_grid():
    from porl_amd.env import AStarExpert, PlanGrid
    world, g = EC.tiny_world(), EC.tiny_grid()
    occ, _ = EC.rasterize(world[0], world[1], g)
    free = np.argwhere(~occ)
    states = EC.state_rows([(*g.centre(*free[k]), 0.3, *g.centre(*free[-1 - k])) for k in range(len(free))])
    w = world_of(world, origin=(0.0, 0.0))
    sim = sim_with(w, states)
    ex = AStarExpert(sim, grid=PlanGrid(w, **g.kwargs()), lookahead=1)
    got = ex.plan(max_path=12)
    pl = EC.Planner(g, occ, lookahead=1)
    want = pl.act(states, max_path=12)
    rows = device_rows(ex)
    for i in range(len(states)):
        assert np.array_equal(rows[i], raw_field(pl.field_of(tuple(free[-1 - i])), g)), i
    assert np.array_equal(host(got.status), want["status"]) and np.array_equal(host(got.path_len), want["path_len"])
    assert np.array_equal(host(got.path), want["path"]) and np.array_equal(host(got.waypoint), want["waypoint"])
    assert (want["status"] == EC.OK).any()


# ---- the reference's paths: the largest LDS footprint, 20 cells per thread -------------------------------------------------------
def _scene(k):
    z, _ = load_golden("expert_paths")
    g = EC.GOLDEN_GRID
    occ = np.unpackbits(z["occ"][k])[:g.w * g.h].reshape(g.w, g.h).astype(bool)
    n = int(z["offsets"][k + 1] - z["offsets"][k])
    return str(z["kind"][k]), occ, tuple(int(v) for v in z["start"][k]), tuple(int(v) for v in z["goal"][k]), n


@pytest.mark.parametrize("k", range(11))
def test_paths_match_the_restatement_and_the_reference(k):
    from porl_amd.env import AStarExpert, NavWorld, PlanGrid
    kind, occ, start, goal, len_rx = _scene(k)
    g = EC.GOLDEN_GRID
    empty = NavWorld(np.zeros((0, 4), np.float32), origin=(g.min_x, g.min_y)).to(DEV)
    grid = PlanGrid(empty, **g.kwargs())
    assert not bool(grid.occupancy().any())
    grid.bitmap.copy_(torch.from_numpy(EC.pack_bitmap(occ).view(np.int32)))         # the scene's occupancy, as recorded
    assert np.array_equal(host(grid.occupancy()), occ)
    st = EC.state_rows([(*g.centre(*start), 0.4, *g.centre(*goal))])
    sim = sim_with(empty, st)                                                       # N = 1
    pl = EC.Planner(g, occ)
    want = pl.act(st, max_path=len_rx + 2)
    ex = AStarExpert(sim, grid=grid)
    got = ex.plan(max_path=len_rx + 2)
    sealed = kind == "sealed_start"
    assert int(got.path_len[0]) == (0 if sealed else len_rx), kind                  # len(rx); the reference's lone goal node
    assert int(got.status[0]) == (EC.NO_FIELD if sealed else EC.OK)
    assert np.array_equal(device_rows(ex)[0], raw_field(pl.field_of(goal), g))      # every cell of the field
    for name in ("status", "path_len", "path", "waypoint"):
        assert np.array_equal(host(getattr(got, name)), want[name]), (kind, name)
    if not sealed:
        assert host(got.path)[0, 0].tolist() == list(start) and host(got.path)[0, len_rx - 1].tolist() == list(goal)
        assert (host(got.path)[0, len_rx:] == -1).all()
        # max_path shorter than the path: truncated, nothing written past it
        short = max(len_rx // 2, 1)
        cut = ex.plan(max_path=short)
        assert cut.path.shape == (1, short, 2) and np.array_equal(host(cut.path), want["path"][:, :short])
        assert int(cut.path_len[0]) == len_rx
        # a lookahead longer than the path: the waypoint is the goal position itself
        far = AStarExpert(sim, grid=grid, lookahead=len_rx + 5).plan()
        assert np.array_equal(host(far.waypoint)[0], st[0, 3:5]) and int(far.path_len[0]) == len_rx
    assert ex.plan().path is None


# ---- steer ----------------------------------------------------------------------------------------------------------------
def test_commands_and_scores_match_the_restatement():
    from porl_amd.env import AStarExpert
    world, g = EC.lattice_world(), EC.lattice_grid()
    occ, _ = EC.rasterize(world[0], world[1], g)
    pl = EC.Planner(g, occ)
    states = EC.random_states(96, 5, g, occ, pl)
    want = pl.act(states, max_path=8)
    assert pl.margin > EC.MARGIN and (want["status"] == EC.OK).all()
    w = world_of(world)
    ex = AStarExpert(sim_with(w, states))
    assert_steer(host(ex()), want["commands"], "commands")
    got = ex.plan(max_path=8)
    for name in ("status", "path_len", "path", "waypoint"):
        assert np.array_equal(host(getattr(got, name)), want[name]), name
    dx = AStarExpert(sim_with(w, states, discrete=True))
    scores = host(dx())
    assert scores.shape == (96, 5) and scores.dtype == np.float32
    assert_steer(scores, want["scores"], "scores")
    keep = EC.gap_rows(want["scores"])
    print(f"scores: {int((~keep).sum())} of 96 rows under the gap")
    assert (~keep).mean() < 0.02
    assert np.array_equal(scores.argmax(1)[keep], want["scores"].argmax(1)[keep])
    # the same through the epsilon-greedy rule at epsilon 0: the nearest turn
    from porl_amd import engine as E
    act = host(E.qnet_select(dx(), 0.0, 3, 0))
    assert np.array_equal(act[keep], want["scores"].argmax(1)[keep])
    # another lookahead moves the waypoint
    pl3 = EC.Planner(g, occ, lookahead=3)
    assert np.array_equal(host(AStarExpert(sim_with(w, states), lookahead=3).plan().waypoint), pl3.act(states)["waypoint"])
    out = torch.empty(96, 2, dtype=torch.float32, device=DEV)
    assert ex(out=out) is out and torch.equal(out, ex(ex.sim.obs))


def test_every_status_and_its_fallback():
    from porl_amd.env import AStarExpert
    world, g = EC.room_world(), EC.lattice_grid()
    occ, _ = EC.rasterize(world[0], world[1], g)
    states = EC.status_states()
    pl = EC.Planner(g, occ)
    want = pl.act(states, max_path=6)
    assert want["status"].tolist() == EC.STATUS_WANT and pl.margin > EC.MARGIN
    w = world_of(world)
    ex = AStarExpert(sim_with(w, states))
    got = ex.plan(max_path=6)
    assert host(got.status).tolist() == EC.STATUS_WANT
    assert np.array_equal(host(got.path_len), want["path_len"]) and np.array_equal(host(got.path), want["path"])
    assert np.array_equal(host(got.waypoint), want["waypoint"], equal_nan=True)
    bad = want["status"] != EC.OK
    assert (host(got.path_len)[bad] == 0).all() and (host(got.path)[bad] == -1).all()
    assert np.array_equal(host(got.waypoint)[bad], states[bad, 3:5], equal_nan=True)     # straight at the goal
    cmd = host(ex())
    assert_steer(cmd, want["commands"], "status commands")
    nf = want["status"] == EC.NON_FINITE
    assert (cmd[nf] == 0).all()
    scores = host(AStarExpert(sim_with(w, states, discrete=True))())
    assert_steer(scores, want["scores"], "status scores")
    assert (scores[nf] == 0).all()


# ---- the cache in a roll-out ------------------------------------------------------------------------------------------------
def test_cache_follows_the_goals_in_a_rollout():
    from porl_amd.env import AStarExpert, LidarNavSim
    world, g = EC.lattice_world(), EC.lattice_grid()
    occ, _ = EC.rasterize(world[0], world[1], g)
    pl = EC.Planner(g, occ)
    sim = LidarNavSim(world_of(world), 64, seed=NC.ROLLOUT["seed"], auto_reset=True, episode_step=40)
    sim.reset()
    ex = AStarExpert(sim)
    refreshed = kept = 0
    for t in range(60):
        states = host(sim.state)
        cells = [pl.goal_cell(st) for st in states]
        assert all(s == EC.OK for s, _ in cells)
        names = np.array([c[1] * g.w + c[0] + 1 for _, c in cells])
        fields0, tags0 = ex.fields.clone(), host(ex.tags)
        a = ex(sim.obs)
        want = pl.act(states)
        assert (want["status"] == EC.OK).all()
        assert_steer(host(a), want["commands"], f"step {t}")
        same = tags0 == names
        assert np.array_equal(host(ex.tags), names)
        keep = torch.from_numpy(same).to(DEV)
        assert torch.equal(ex.fields[keep], fields0[keep])                         # an unchanged goal cell: the field stays
        rows = host(ex.fields[~keep]).view(np.uint32)
        for r, i in zip(rows, np.flatnonzero(~same)):
            assert np.array_equal(r, raw_field(pl.field_of(cells[i][1]), g)), (t, i)
        refreshed, kept = refreshed + int((~same).sum()), kept + int(same.sum())
        sim.step(a)
    print(f"roll-out: {refreshed} fields refreshed, {kept} kept, smallest margin {pl.margin:.3e}")
    assert pl.margin > EC.MARGIN
    assert refreshed >= 2 * 64 and kept > 40 * 64              # every robot met a second goal; most calls relax nothing


def test_one_simulator_of_64_equals_two_of_32():
    from porl_amd.env import AStarExpert, LidarNavSim
    w = world_of(EC.lattice_world())
    kw = dict(seed=77, auto_reset=True, episode_step=12)
    whole = LidarNavSim(w, 64, **kw)
    halves = [LidarNavSim(w, 32, env_offset=o, **kw) for o in (0, 32)]
    experts = [AStarExpert(s) for s in (whole, *halves)]
    for s in (whole, *halves):
        s.reset()
    for _ in range(30):
        a = [e() for e in experts]
        assert torch.equal(a[0], torch.cat(a[1:]))
        for s, c in zip((whole, *halves), a):
            s.step(c)
        assert torch.equal(whole.state, torch.cat([h.state for h in halves]))
    assert torch.equal(experts[0].fields, torch.cat([e.fields for e in experts[1:]]))
    assert torch.equal(experts[0].tags, torch.cat([e.tags for e in experts[1:]]))
    assert int(whole.counters[:, 1].min()) >= 2                # every robot was reset on the way


# ---- behaviour --------------------------------------------------------------------------------------------------------------
def test_the_continuous_expert_reaches_its_goals():
    from porl_amd.env import AStarExpert, LidarNavSim
    from porl_amd.evaluate import evaluate_policy_batched
    sim = LidarNavSim(world_of(EC.lattice_world()), 256)
    steps, score, success = evaluate_policy_batched(AStarExpert(sim), sim, 256, 300)
    print(f"continuous expert: success {success:.4f}, mean steps {steps:.1f}, mean score {score:.1f}")
    assert success >= 0.9


def test_the_discrete_expert_reaches_its_goals_through_collect_discrete():
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.env import AStarExpert, DiscreteLidarNavSim
    from porl_amd.train.vector_offline import collect_discrete
    sim = DiscreteLidarNavSim(world_of(EC.lattice_world()), 256, auto_reset=True)
    replay = DeviceReplay(1024, sim.obs_dim)
    out = collect_discrete(sim, replay, 300, epsilon=0.0, expert=AStarExpert(sim))
    episodes, _, goals, hits = out["tallies"]
    print(f"discrete expert: {int(episodes)} episodes, {int(goals)} goals, {int(hits)} hits: {goals / episodes:.4f}")
    assert out["transitions"] == 256 * 300 and episodes >= 256 and goals >= 0.8 * episodes
    with pytest.raises(ValueError, match="not both"):
        collect_discrete(sim, replay, 1, trainer=object(), expert=AStarExpert(sim))


def test_epsilon_one_is_the_random_policy_action_for_action():
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.env import AStarExpert, DiscreteLidarNavSim
    from porl_amd.train.vector_offline import collect_discrete
    w = world_of(EC.lattice_world())
    actions = []
    for with_expert in (False, True):
        sim = DiscreteLidarNavSim(w, 64, seed=5, auto_reset=True)
        replay = DeviceReplay(64 * 20, sim.obs_dim)
        collect_discrete(sim, replay, 20, epsilon=1.0, seed=9, expert=AStarExpert(sim) if with_expert else None)
        actions.append(replay.actions.clone())
    assert torch.equal(actions[0], actions[1]) and len(torch.unique(actions[0])) == 5


def test_cache_limit_and_devices():
    from porl_amd import _native as N
    from porl_amd.env import AStarExpert, LidarNavSim
    sim = LidarNavSim(world_of(EC.lattice_world()), 4)
    with pytest.raises(ValueError, match=str(4 * 2809 * 4)):
        AStarExpert(sim, max_cache_bytes=4 * 2809 * 4 - 1)
    AStarExpert(sim, max_cache_bytes=4 * 2809 * 4)
    with pytest.raises(ValueError, match="lookahead"):
        AStarExpert(sim, lookahead=0)
    with pytest.raises(N.NativeError, match="no CPU path"):
        AStarExpert(sim)(out=torch.empty(4, 2))
