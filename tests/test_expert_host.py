"""The A* expert without a GPU: the numpy restatement (tests/helpers/expert_cases.py) against the paths the reference's own
`AStarPlanner.planning` returned (tests/golden/expert_paths.npz, written by tests/helpers/gen_expert_golden.py), closed
forms of the rasteriser and the descent, every status, a roll-out of the restated expert on the host simulator, every
rejected argument of the two entry points (through ctypes and in a stand-alone program under the host sanitizers), and the
Python layer's refusal to run on the CPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden
from helpers import expert_cases as EC
from helpers import navsim_cases as NC
from porl_amd import _native as N

ENTRY_POINTS = ("porl_nav_rasterize", "porl_nav_expert")


def test_abi_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(", txt), name
        assert name in N.SYMBOLS
        assert hasattr(N.lib(), name)
    assert re.search(r"#define\s+PORL_ABI_VERSION\s+12\b", txt)                    # additions only
    assert N.ABI_VERSION == 12 and N.lib().porl_abi_version() == 12
    # the ctypes mirrors have the header's fields in the header's order
    for struct, mirror, size in (("porl_nav_grid", N.NavGrid, 4 * 8 + 2 * 4), ("porl_nav_expert_params", N.NavExpertParams, 4 * 8 + 4 * 4)):
        body = txt.split(f"typedef struct {struct} {{")[1].split(f"}} {struct};")[0]
        fields = []
        for kind, names in re.findall(r"^\s*(double|int32_t)\s+([\w, ]+);", body, re.M):
            fields += [n.strip() for n in names.split(",")]
        assert fields == [f[0] for f in mirror._fields_], struct
        assert C.sizeof(mirror) == size
    for k, name in enumerate(("OK", "NO_FIELD", "GOAL_OFF_GRID", "GOAL_BLOCKED", "NON_FINITE", "NOT_CONVERGED")):
        assert re.search(rf"#define\s+PORL_EXPERT_{name}\s+{k}\b", txt)
        assert getattr(EC, name) == k
    from porl_amd.env import expert as X
    assert X.STATUS_NAMES == ("ok", "no_field", "goal_off_grid", "goal_blocked", "non_finite", "not_converged")


# ---- the restatement against the reference's recorded paths -----------------------------------------------------------------
def _golden():
    z, _ = load_golden("expert_paths")
    g = EC.GOLDEN_GRID
    for k, kind in enumerate(z["kind"]):
        occ = np.unpackbits(z["occ"][k])[:g.w * g.h].reshape(g.w, g.h).astype(bool)
        lo, hi = z["offsets"][k], z["offsets"][k + 1]
        # the reference returns positions, goal first: back to cells, start first
        ix = np.rint((z["rx"][lo:hi] - g.min_x) / g.res).astype(int)[::-1]
        iy = np.rint((z["ry"][lo:hi] - g.min_y) / g.res).astype(int)[::-1]
        yield str(kind), occ, tuple(int(v) for v in z["start"][k]), tuple(int(v) for v in z["goal"][k]), list(zip(ix, iy))


def _moves(path):
    """(axis moves, diagonal moves) of a cell path; asserts it is 8-connected."""
    a = b = 0
    for (x0, y0), (x1, y1) in zip(path[:-1], path[1:]):
        dx, dy = abs(x1 - x0), abs(y1 - y0)
        assert max(dx, dy) == 1, (x0, y0, x1, y1)
        a, b = a + (dx + dy == 1), b + (dx + dy == 2)
    return a, b


def test_golden_covers_the_situations():
    scenes = {kind: (occ, s, g, ref) for kind, occ, s, g, ref in _golden()}
    assert len(scenes) >= 11
    assert len(scenes["detour"][3]) > 100                                           # a detour of more than 100 nodes
    assert _moves(scenes["diagonal"][3])[0] == 0                                    # a diagonal-only path
    assert len(scenes["adjacent_axis"][3]) == 2 and len(scenes["same_cell"][3]) == 1
    assert scenes["walls_with_gaps"][0].any() and not scenes["open"][0].any()
    for kind, (occ, s, g, ref) in scenes.items():
        assert not occ[s] and not occ[g], kind                                      # start and goal cells are free
        assert occ.shape == (200, 100)


def test_restated_paths_against_the_reference():
    sealed = 0
    for kind, occ, start, goal, ref in _golden():
        fld = EC.field(occ, goal)
        mine = EC.descend(fld, start, goal)
        if kind == "sealed_start":
            # no path: the reference's open set runs empty and it returns the lone goal node; here that is NO_FIELD, length 0
            assert ref == [goal] and start != goal and mine == [], kind
            pl = EC.Planner(EC.GOLDEN_GRID, occ)
            st = EC.state_rows([(*EC.GOLDEN_GRID.centre(*start), 0.0, *EC.GOLDEN_GRID.centre(*goal))])[0]
            q = pl.plan(st)
            assert q["status"] == EC.NO_FIELD and q["path_len"] == 0
            sealed += 1
            continue
        assert len(mine) == len(ref), (kind, len(mine), len(ref))                   # path_len == len(rx)
        assert ref[0] == start and ref[-1] == goal and mine[0] == start and mine[-1] == goal
        # the reference's own path, walked from start to goal, is a valid descent of the restated field
        for c, n in zip(ref[:-1], ref[1:]):
            move = 0x10000 if (n[0] - c[0] == 0 or n[1] - c[1] == 0) else 1
            assert int(fld[n]) + move == int(fld[c]), (kind, c, n)
        # the restated path is 8-connected, touches no blocked cell and has the same (a, b)
        assert not any(occ[c] for c in mine), kind
        a, b = _moves(mine)
        assert (a, b) == _moves(ref) == (int(fld[start]) >> 16, int(fld[start]) & 0xFFFF), kind
        # the planner's answer for a robot on the start cell's centre
        pl = EC.Planner(EC.GOLDEN_GRID, occ)
        st = EC.state_rows([(*EC.GOLDEN_GRID.centre(*start), 0.0, *EC.GOLDEN_GRID.centre(*goal))])[0]
        q = pl.plan(st, max_path=len(ref) + 3)
        assert q["status"] == EC.OK and q["path_len"] == len(ref)
        assert [tuple(c) for c in q["path"][:len(ref)]] == mine and (q["path"][len(ref):] == -1).all()
    assert sealed == 1


# ---- closed forms ---------------------------------------------------------------------------------------------------------
def test_a_point_obstacle_blocks_exactly_the_cells_within_inflate():
    g = EC.Grid(0.5, 1.2, 0.0, 0.0, 9, 9)                      # (i^2 + j^2) / 4 <= 1.44: i^2 + j^2 <= 5, no tie (5.76)
    want = np.array([[(i - 4) ** 2 + (j - 4) ** 2 <= 5 for j in range(9)] for i in range(9)])
    occ, m = EC.rasterize(np.zeros((0, 4)), [[2.0, 2.0, 0.0]], g)
    assert np.array_equal(occ, want) and want.sum() == 21 and m > 0.08
    # a degenerate segment is the same point; a pillar of radius r is the point inflated by r more
    occ2, _ = EC.rasterize([[2.0, 2.0, 2.0, 2.0]], np.zeros((0, 3)), g)
    assert np.array_equal(occ2, want)
    occ3, _ = EC.rasterize(np.zeros((0, 4)), [[2.0, 2.0, 0.5]], EC.Grid(0.5, 0.7, 0.0, 0.0, 9, 9))
    assert np.array_equal(occ3, want)
    # a segment blocks a stadium: its ends are round
    occ4, _ = EC.rasterize([[1.0, 2.0, 3.0, 2.0]], np.zeros((0, 3)), EC.Grid(0.5, 0.6, 0.0, 0.0, 9, 9))
    assert occ4[2:7, 3:6].all() and occ4[1, 4] and not occ4[1, 3] and not occ4[0, 4] and occ4.sum() == 17
    # the bitmap layout, there and back
    words = EC.pack_bitmap(want)
    assert words.dtype == np.uint32 and len(words) == (11 * 11 + 31) // 32
    assert np.array_equal(EC.unpack_interior(words, g), want)
    p = (4 + 1) * 11 + 4 + 1
    assert (words[p >> 5] >> (p & 31)) & 1


def test_descent_closed_forms():
    g = EC.Grid(1.0, 0.0, 0.0, 0.0, 9, 7)
    occ = np.zeros((9, 7), bool)
    fld = EC.field(occ, (6, 3))
    a, b = EC.pairs(fld)
    assert (a[0, 0], b[0, 0]) == (3, 3) and (a[6, 3], b[6, 3]) == (0, 0) and (a[8, 6], b[8, 6]) == (1, 2)
    # motion order: axis moves first ((1, 0) before the diagonals), so (0, 0) -> (6, 3) starts along x
    assert EC.descend(fld, (0, 0), (6, 3)) == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (5, 2), (6, 3)]
    pl = EC.Planner(g, occ, lookahead=2)
    q = pl.plan(EC.state_rows([(0.2, -0.1, 0.0, 6.3, 2.9)])[0], max_path=4)
    assert q["status"] == EC.OK and q["path_len"] == 7 and q["waypoint"] == (2.0, 0.0)
    assert q["path"].tolist() == [[0, 0], [1, 0], [2, 0], [3, 0]]                   # truncated, nothing past max_path
    # inside the lookahead the waypoint is the goal position itself, not the cell centre
    for start in ((5.1, 2.2), (6.0, 2.8), (6.2, 3.1)):
        q = pl.plan(EC.state_rows([(*start, 0.0, 6.3, 2.9)])[0])
        assert q["status"] == EC.OK and q["waypoint"] == (6.3, 2.9)
    assert EC.Planner(g, occ, lookahead=50).plan(EC.state_rows([(0.2, -0.1, 0.0, 6.3, 2.9)])[0])["waypoint"] == (6.3, 2.9)
    # a blocked start cell: the first step goes to its reached neighbour of least cost, ties to the motion order
    occ[2, 2] = True
    pl = EC.Planner(g, occ, lookahead=1)
    q = pl.plan(EC.state_rows([(2.0, 2.0, 0.0, 6.0, 2.0)])[0], max_path=8)
    assert EC.field(occ, (6, 2))[2, 2] == EC.UNREACHED
    assert q["status"] == EC.OK and q["path"][:2].tolist() == [[2, 2], [3, 2]] and q["path_len"] == 5
    assert q["waypoint"] == (3.0, 2.0)                                              # the neighbour counts as the first step
    q = pl.plan(EC.state_rows([(2.0, 2.0, 0.0, 2.0, 6.0)])[0], max_path=8)          # goal straight up: (2, 3) is nearest
    assert q["path"][:2].tolist() == [[2, 2], [2, 3]] and q["path_len"] == 5
    # equal costs: (3, 3) and (3, 1) both lie 3 axis moves from (6, 2)... and (3, 2) beats both; block it too
    occ[3, 2] = True
    q = EC.Planner(g, occ, lookahead=1).plan(EC.state_rows([(2.0, 2.0, 0.0, 6.0, 2.0)])[0], max_path=8)
    assert q["path"][1].tolist() == [3, 1]                     # (1, -1) comes before (1, 1) in the motion order


def test_every_status():
    world = EC.room_world()
    g = EC.lattice_grid()
    occ, m = EC.rasterize(*world, g)
    assert m > EC.MARGIN
    assert not occ[24:27, 24:27].any() and occ[21:24, 21:30].all() and occ[27:30, 21:30].all()   # the room and its ring
    pl = EC.Planner(g, occ)
    states = EC.status_states()
    got = pl.act(states, max_path=6)
    assert got["status"].tolist() == EC.STATUS_WANT
    assert pl.margin > EC.MARGIN
    bad = got["status"] != EC.OK
    # every status but OK: the waypoint is the goal position itself, no path
    assert (got["path_len"][bad] == 0).all() and (got["path"][bad] == -1).all()
    w, s = got["waypoint"][bad], states[bad, 3:5]
    assert np.array_equal(w[~np.isnan(w)], s[~np.isnan(s)]) and np.array_equal(np.isnan(w), np.isnan(s))
    nf = got["status"] == EC.NON_FINITE
    assert (got["commands"][nf] == 0).all() and (got["scores"][nf] == 0).all()
    # ... and the command steers straight at it
    for i in np.flatnonzero(bad & ~nf):
        e = math.atan2(states[i, 4] - states[i, 1], states[i, 3] - states[i, 0]) - states[i, 2]
        e = (e + math.pi) % (2 * math.pi) - math.pi
        assert abs(got["commands"][i, 1] - min(max(e / 0.2, -1.5), 1.5)) < 1e-12
        assert abs(got["commands"][i, 0] - 0.15 * max(0.0, math.cos(e))) < 1e-12
    assert got["path_len"][11] == 1 and got["path_len"][7] >= 36 and got["path"][7, 0].tolist() == [11, 12]
    # scores: the arg-max is the turn nearest the heading error
    e = np.array([pl.error(st, wp) for st, wp in zip(states[~nf], got["waypoint"][~nf])])
    turns = (2 - np.arange(5)) * 0.75 * 0.2
    assert np.array_equal(got["scores"][~nf].argmax(1), np.abs(e[:, None] - turns).argmin(1))


def test_case_generators_keep_their_margins():
    g = EC.lattice_grid()
    occ, m = EC.rasterize(*EC.lattice_world(), g)
    assert m > EC.MARGIN and occ.sum() == 2 * 4 * 51 - 16 + 16 * 21              # two rows along each wall, 21 cells a pillar
    _, m = EC.rasterize(*NC.oblique(), EC.oblique_grid())
    assert m > EC.MARGIN
    tocc, m = EC.rasterize(*EC.tiny_world(), EC.tiny_grid())
    assert m > EC.MARGIN and tocc.any() and not tocc.all()
    pl = EC.Planner(g, occ)
    states = EC.random_states(96, 5, g, occ, pl)
    got = pl.act(states)
    assert pl.margin > EC.MARGIN and (got["status"] == EC.OK).all()
    keep = EC.gap_rows(got["scores"])
    assert (~keep).mean() < 0.02                               # score ties: under 2 % of a case


def test_rollout_of_the_restated_expert_on_the_host():
    """32 lattice episodes of the host simulator driven by the restated expert (inflate 0.18, lookahead 2): at least 29
    reach the goal.  (A 200-episode prototype of these rules reached 199.)"""
    world = NC.lattice()
    p = NC.params()
    sim = NC.Sim(world, 32, seed=7, auto_reset=False, p=p)
    sim.reset()
    g = EC.lattice_grid(origin=(p["origin_x"], p["origin_y"]))
    occ, _ = EC.rasterize(*world, g)
    pl = EC.Planner(g, occ, lookahead=2)
    for _ in range(p["episode_step"]):
        run = np.flatnonzero((sim.counters[:, 2] & 0xff) == NC.RUNNING)
        if not len(run):
            break
        a = np.zeros((32, 2), np.float32)
        for i in run:
            a[i] = pl.command(sim.state[i], pl.plan(sim.state[i]))
        sim.step(a)
    status = sim.counters[:, 2] & 0xff
    goals, hits = int((status == NC.GOAL).sum()), int((status == NC.HIT).sum())
    print(f"host roll-out: {goals} goals, {hits} hits of 32")
    assert goals >= 29


# ---- rejected arguments ---------------------------------------------------------------------------------------------------
_F = (C.c_float * 4096)()
_D = (C.c_double * 4096)()
_I = (C.c_int64 * 4096)()


def _grid(**over):
    a = dict(resolution=0.1, inflate=0.18, min_x=-10.0, min_y=5.0, w=51, h=51)
    a.update(over)
    return N.NavGrid(**a)


def _ep(**over):
    a = dict(dt=0.2, max_lin_vel=0.15, max_ang_vel=1.5, ang_step=0.75, n_actions=5, lookahead=2, max_path=0, reserved=0)
    a.update(over)
    return N.NavExpertParams(**a)


def _rast(**over):
    a = dict(segments=_F, M=4, circles=_F, C=16, grid=_grid(), bitmap=_I, n_words=88)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_nav_rasterize(a["segments"], a["M"], a["circles"], a["C"], a["grid"], a["bitmap"], a["n_words"], None)
    return rc, lib.porl_last_error().decode()


def _expert(**over):
    a = dict(grid=_grid(), bitmap=_I, params=_ep(), state=_D, field=_I, tag=_I, commands=_F, cmd_stride=2, scores=None,
             score_stride=0, n=4)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_nav_expert(a["grid"], a["bitmap"], a["params"], a["state"], a["field"], a["tag"], a["commands"],
                             a["cmd_stride"], a["scores"], a["score_stride"], None, None, None, None, a["n"], None)
    return rc, lib.porl_last_error().decode()


@pytest.mark.parametrize("fn,over,word", [
    (_rast, dict(M=2040, C=9), "primitives"), (_rast, dict(segments=None), "null segments"), (_rast, dict(grid=None), "null grid"),
    (_rast, dict(bitmap=None), "null bitmap"), (_rast, dict(n_words=87), "n_words"),
    (_rast, dict(grid=_grid(resolution=0.0)), "resolution"), (_rast, dict(grid=_grid(inflate=-0.1)), "inflate"),
    (_rast, dict(grid=_grid(w=300, h=300)), "grid"), (_rast, dict(grid=_grid(w=254, h=254)), "LDS"),
    (_rast, dict(grid=_grid(w=65533, h=2)), "grid"), (_rast, dict(grid=_grid(w=0)), "grid"),
    (_expert, dict(bitmap=None), "null bitmap"), (_expert, dict(params=None), "null params"), (_expert, dict(state=None), "null state"),
    (_expert, dict(field=None), "null field"), (_expert, dict(tag=None), "null tag"), (_expert, dict(n=0), "n 0"),
    (_expert, dict(params=_ep(lookahead=0)), "lookahead"), (_expert, dict(params=_ep(max_path=-1)), "max_path"),
    (_expert, dict(grid=_grid(resolution=-1.0)), "resolution"), (_expert, dict(grid=_grid(inflate=-1.0)), "inflate"),
    (_expert, dict(grid=_grid(w=300, h=300)), "grid"), (_expert, dict(cmd_stride=1), "cmd_stride"),
    (_expert, dict(commands=None, cmd_stride=0, scores=_F, score_stride=5, params=_ep(n_actions=0)), "n_actions"),
    (_expert, dict(commands=None, cmd_stride=0, scores=_F, score_stride=65, params=_ep(n_actions=65)), "n_actions"),
    (_expert, dict(commands=None, cmd_stride=0, scores=_F, score_stride=4), "score_stride"),
    (_expert, dict(params=_ep(dt=0.0)), "dt"),
])
def test_bad_arguments_are_rejected_by_name(fn, over, word):
    rc, msg = fn(**over)
    assert rc == -1 and word in msg, (rc, msg)


def test_rejected_arguments_under_sanitizers():
    """tests/helpers/abi_reject_expert.cpp on the host-only sanitized build: every rejected argument of the two entry
    points comes back as PORL_ERR_INVALID with a message that names it, before any HIP call; ASan / UBSan abort the process
    on any finding.  A stand-alone program: nothing sanitized is loaded into this interpreter."""
    from porl_amd import build as Bd
    assert Bd.build_sanitized_expert(verbose=False) == Bd.SAN_EXPERT_DRIVER
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([Bd.SAN_EXPERT_DRIVER], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "0 unexpected" in r.stdout
    assert int(r.stdout.split("abi_reject_expert:")[1].split("checks")[0]) >= 55


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def test_python_surface_has_no_cpu_path():
    import inspect
    from porl_amd.env import AStarExpert, NavWorld, PlanGrid
    from porl_amd.train.vector_offline import collect_discrete
    with pytest.raises(N.NativeError, match="no CPU path"):
        PlanGrid(NavWorld.lattice())                                               # a world on the CPU
    with pytest.raises(ValueError, match="origin"):
        PlanGrid(NavWorld(np.zeros((1, 4), np.float32)))
    assert "privileged" in AStarExpert.__call__.__doc__
    sig = inspect.signature(collect_discrete)
    assert sig.parameters["expert"].default is None and list(sig.parameters)[:7] == ["sim", "replay", "n_steps", "trainer",
                                                                                      "epsilon", "seed", "t0"]
    with pytest.raises(ValueError, match="not both"):
        collect_discrete(None, None, 1, trainer=object(), expert=object())
    d = inspect.signature(PlanGrid).parameters
    assert (d["resolution"].default, d["inflate"].default, d["cells"].default) == (0.1, 0.18, 5)
    assert inspect.signature(AStarExpert).parameters["lookahead"].default == 2
    assert inspect.signature(AStarExpert).parameters["max_cache_bytes"].default == 1 << 30
