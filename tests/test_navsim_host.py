"""The lidar navigation simulator without a GPU: the numpy restatement (tests/helpers/navsim_cases.py) against what the
reference's own `getSarsa` and `random_pts_map` returned (tests/golden/navsim_sarsa.npz, navsim_reset.npz, written by
tests/helpers/gen_navsim_golden.py), closed forms of the ray cast, the roll-out the GPU tests repeat, every rejected
argument of the three entry points (through ctypes and in a stand-alone program under the host sanitizers), and the
Python layer's refusal to run on the CPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden
from helpers import navsim_cases as NC
from porl_amd import _native as N

ENTRY_POINTS = ("porl_nav_scan", "porl_nav_reset", "porl_nav_step")


def test_abi_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(", txt), name
        assert name in N.SYMBOLS
        assert hasattr(N.lib(), name)
    assert re.search(r"#define\s+PORL_ABI_VERSION\s+12\b", txt)                    # additions only
    assert N.ABI_VERSION == 12 and N.lib().porl_abi_version() == 12
    # the ctypes mirror has the header's fields in the header's order
    body = txt.split("typedef struct porl_nav_params {")[1].split("} porl_nav_params;")[0]
    fields = re.findall(r"^\s*(?:double|int32_t)\s+(\w+);", body, re.M)
    assert fields == [f[0] for f in N.NavParams._fields_]
    assert C.sizeof(N.NavParams) == 16 * 8 + 6 * 4


# ---- the restatement against the reference's recorded results -------------------------------------------------------------
def test_sarsa_matches_the_reference():
    z, _ = load_golden("navsim_sarsa")
    n = len(z["reward"])
    assert n >= 200 and np.isinf(z["scan"]).any() and np.isnan(z["scan"]).any()
    assert set(np.unique(z["status"])) == {0, 1, 2}
    for k in range(n):
        st = np.array([*z["pose"][k], *z["goal"][k], *z["prev"][k], 0.0])
        rx, ry, r, term, stat, _ = NC.sarsa(st, z["scan"][k])
        state = z["state"][k]
        scan = np.where(np.isfinite(z["scan"][k]), z["scan"][k], np.float32(10.0)).astype(np.float64)
        assert np.array_equal(state[:360], scan)
        assert abs(rx - state[360]) <= 1e-12 and abs(ry - state[361]) <= 1e-12
        assert abs(r - z["reward"][k]) <= 1e-12, (k, r, z["reward"][k])
        assert term == bool(z["terminated"][k]) and stat == int(z["status"][k])                   # decisions exact
        assert np.abs(st[5:7] - z["new_prev"][k]).max() <= 1e-12


def test_reset_draws_match_the_reference():
    z, _ = load_golden("navsim_reset")
    assert len(z["seed"]) == 256
    worst = 0
    for k in range(256):
        x1, y1, x2, y2, j, capped, _ = NC.reset_draw(int(z["seed"][k]), int(z["env"][k]), int(z["episode"][k]))
        assert np.abs(np.array([x1, y1, x2, y2]) - z["xy"][k]).max() <= 1e-12
        assert j == int(z["draws"][k]) and not capped
        worst = max(worst, j)
    assert 8 < worst < NC.MAX_DRAWS                                                # some triples did redraw
    # the spawn rule: coordinates in k + [0.16, 0.84] of the rank-0 square, goal 0.3 .. 3.5 away
    xy = z["xy"] - np.array([-10.0, 5.0, -10.0, 5.0])
    frac = xy - np.floor(xy)
    assert (xy > 0).all() and (xy < 5).all() and (frac > 0.16 - 1e-12).all() and (frac < 0.84 + 1e-12).all()
    d = np.hypot(xy[:, 2] - xy[:, 0], xy[:, 3] - xy[:, 1])
    assert (d >= 0.3).all() and (d <= 3.5).all()


def test_sm64_is_the_librarys():
    # the finaliser of csrc/episodes.hpp (ep_sm64), on its published test value and a wrap-around
    assert NC.sm64(0) == 0xE220A8397B1DCDAF
    assert NC.sm64((1 << 64) - 1) == NC.sm64(-1 & NC.M64)
    assert 0.0 <= NC.u01(NC.robot_key(3, 4), 5, 6) < 1.0


# ---- closed forms ---------------------------------------------------------------------------------------------------------
def test_cast_closed_forms():
    none = np.zeros((0, 3), np.float32)
    # a single wall at distance D: D / cos
    wall = np.array([[2, -50, 2, 50]], np.float32)
    r = NC.cast(wall, none, [[0.0, 0.0, 0.0]])[0].astype(np.float64)
    for i in range(-49, 50, 7):                        # 2 / cos(49 deg) = 3.05 < range_max
        want = 2.0 / math.cos(math.radians(i))
        assert abs(r[i % 360] - want) <= 2.5e-7 * want
    assert (r[91:270] == 10.0).all()
    assert r[75] == 10.0                                    # 2 / cos(75 deg) = 7.7 > range_max
    # the same wall seen by a turned robot: beam i looks along yaw + i degrees
    r2 = NC.cast(wall, none, [[0.0, 0.0, math.radians(30)]])[0]
    assert abs(float(r2[330]) - 2.0) < 1e-6 and abs(float(r2[0]) - 2.0 / math.cos(math.radians(30))) < 1e-6
    # a pillar dead ahead: dist - r; behind: nothing; from inside a pillar only the far side would be hit: not seen
    pil = np.array([[1.5, 0.0, 0.25]], np.float32)
    r = NC.cast(np.zeros((0, 4), np.float32), pil, [[0.0, 0.0, 0.0]])[0]
    assert abs(float(r[0]) - 1.25) < 1e-7 and r[180] == 10.0
    half = math.degrees(math.asin(0.25 / 1.5))             # the pillar's angular half-width: 9.59 deg
    assert (r[:10] < 10).all() and (r[10:351] == 10.0).all() and (r[351:] < 10).all() and 9 < half < 10
    assert (NC.cast(np.zeros((0, 4), np.float32), pil, [[1.5, 0.1, 0.0]])[0] == 10.0).all()
    # segment ends: a beam past the end misses
    short = np.array([[1.0, -0.1, 1.0, 0.1]], np.float32)
    r = NC.cast(short, none, [[0.0, 0.0, 0.0]])[0]
    assert (r[:6] < 10).all() and (r[6:355] == 10.0).all()   # atan(0.1) = 5.71 deg
    # the nearest primitive wins, a zero range is never returned, beams may be any number
    both = NC.cast(wall, pil, [[0.0, 0.0, 0.0]], NC.params(n_beams=8))
    assert both.shape == (1, 8) and abs(float(both[0, 0]) - 1.25) < 1e-7 and abs(float(both[0, 1]) - 2 * math.sqrt(2)) < 1e-6


def test_lattice_spawn_points_are_clear():
    """With pillar_radius <= 0.096 every spawn point of the reference's rule reads min(scan) >= 0.13: the worst case is
    the cell corner, sqrt(2) * 0.16 - 0.096 = 0.1303."""
    world = NC.lattice(pillar_radius=0.096)
    corners = [[-10 + i + dx, 5 + j + dy, 0.1] for i in range(5) for j in range(5) for dx in (0.16, 0.84) for dy in (0.16, 0.84)]
    assert NC.cast(world[0], world[1], corners).min() >= 0.13
    assert NC.cast(*NC.lattice(pillar_radius=0.1), corners).min() < 0.13


def test_unicycle_step_closed_forms():
    p = NC.PARAMS
    st = [1.0, 2.0, 0.5]
    x, y, yaw = NC.move(st, 0.15, 0.0, p)                                          # straight
    assert abs(x - (1 + 0.03 * math.cos(0.5))) < 1e-15 and abs(y - (2 + 0.03 * math.sin(0.5))) < 1e-15 and yaw == 0.5
    x, y, yaw = NC.move(st, 0.15, 1.5, p)                                          # on the circle of radius v / w
    R = 0.15 / 1.5
    cx, cy = 1.0 - R * math.sin(0.5), 2.0 + R * math.cos(0.5)
    assert abs(math.hypot(x - cx, y - cy) - R) < 1e-15 and abs(yaw - 0.8) < 1e-15
    assert NC.move([0, 0, math.pi - 0.1], 0.0, 1.5, p)[2] == pytest.approx(-math.pi + 0.2, abs=1e-15)   # wrapped once
    assert NC.clip_command([np.nan, np.inf], p) == (0.0, 0.0) and NC.clip_command([9, -9], p) == (0.15, -1.5)


def test_rollout_on_the_host():
    """The roll-out the GPU test repeats: every outcome occurs, no decision within MARGIN of a tie, no spawn under
    min_range, no reset near the draw cap.  (This restatement's commands: outcomes 37 hits, 7 goals, 46 step limits.)"""
    sim, steps, counts = NC.rollout()
    geo, thr, rst = sim.margins()
    print(counts, geo, thr, rst, sim.min_spawn_scan)
    assert counts == {NC.HIT: 37, NC.GOAL: 7, NC.TIMELIMITED: 46}
    assert min(geo, thr, rst) > NC.MARGIN
    assert sim.min_spawn_scan >= 0.13
    assert not (sim.counters[:, 2] & NC.DRAW_CAP).any() and sim.counters[:, 3].max() <= 64
    # rows are [s | r | s' | terminated | a] with s the observation acted on
    first = steps[0]
    assert np.array_equal(first["out"]["rows"][:, :362], first["before"][2])
    assert np.array_equal(first["out"]["rows"][:, 363:725], first["out"]["next_obs"])


# ---- rejected arguments ---------------------------------------------------------------------------------------------------
_F = (C.c_float * 4096)()
_D = (C.c_double * 4096)()
_I = (C.c_int64 * 64)()


def _params(**over):
    p = dict(NC.PARAMS)
    p.update(over)
    return N.NavParams(**p)


def _scan(**over):
    a = dict(segments=_F, M=4, circles=_F, C=16, poses=_D, dirs=_D, params=_params(), out=_F, out_stride=360, n=4)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_nav_scan(a["segments"], a["M"], a["circles"], a["C"], a["poses"], a["dirs"], a["params"], a["out"],
                           a["out_stride"], a["n"], None)
    return rc, lib.porl_last_error().decode()


def _step(**over):
    a = dict(params=_params(), actions=_F, act_stride=2, state=_D, counters=_I, obs=_F, obs_stride=362, next_obs=_D,
             next_stride=362, reward=_F, flags=_I, status=_I, rows=None, row_stride=0, n=4)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_nav_step(_F, 4, _F, 16, _D, a["params"], 1, 0, a["actions"], a["act_stride"], a["state"], a["counters"],
                           a["obs"], a["obs_stride"], a["next_obs"], a["next_stride"], a["reward"], a["flags"], a["status"],
                           a["rows"], a["row_stride"], a["n"], None)
    return rc, lib.porl_last_error().decode()


@pytest.mark.parametrize("fn,over,word", [
    (_scan, dict(M=2040, C=9), "primitives"), (_scan, dict(segments=None), "null segments"),
    (_scan, dict(poses=None), "null poses"), (_scan, dict(out_stride=359), "out_stride"), (_scan, dict(n=0), "n 0"),
    (_scan, dict(params=_params(n_beams=1025)), "n_beams"), (_scan, dict(params=_params(n_beams=0)), "n_beams"),
    (_step, dict(actions=None), "null actions"), (_step, dict(obs_stride=361), "obs_stride"),
    (_step, dict(next_obs=_F), "next_obs must not be obs"), (_step, dict(rows=_F, row_stride=727), "row_stride"),
    (_step, dict(row_stride=728), "without rows"), (_step, dict(params=_params(dt=1.0)), "min_range"),
    (_step, dict(params=_params(dt=0.0)), "dt"), (_step, dict(params=_params(episode_step=0)), "episode_step"),
    (_step, dict(flags=None), "null flags"), (_step, dict(params=_params(layout=1)), "obs_stride"),
])
def test_bad_arguments_are_rejected_by_name(fn, over, word):
    rc, msg = fn(**over)
    assert rc == -1 and word in msg, (rc, msg)


def test_rejected_arguments_under_sanitizers():
    """tests/helpers/abi_reject_navsim.cpp on the host-only sanitized build: every rejected argument of the three entry
    points comes back as PORL_ERR_INVALID with a message that names it, before any HIP call; ASan / UBSan abort the process
    on any finding.  A stand-alone program: nothing sanitized is loaded into this interpreter."""
    from porl_amd import build as Bd
    assert Bd.build_sanitized_navsim(verbose=False) == Bd.SAN_NAVSIM_DRIVER
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([Bd.SAN_NAVSIM_DRIVER], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "0 unexpected" in r.stdout
    assert int(r.stdout.split("abi_reject_navsim:")[1].split("checks")[0]) >= 70


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def test_python_surface_has_no_cpu_path():
    import torch
    from porl_amd import ops as O
    from porl_amd.env import LidarNavSim, NavWorld, nav_scan
    w = NavWorld.lattice()
    assert w.segments.shape == (4, 4) and w.circles.shape == (16, 3) and w.origin == (-10.0, 5.0)
    assert np.array_equal(w.segments.numpy(), NC.lattice()[0]) and np.array_equal(w.circles.numpy(), NC.lattice()[1])
    assert NavWorld.lattice(rank=5).origin == (-5.0, 0.0)                          # env/gazebo.py:298-299
    with pytest.raises(N.NativeError, match="no CPU path"):
        LidarNavSim(w, 4, device="cpu")
    with pytest.raises(N.NativeError, match="no CPU path"):
        nav_scan(w.segments, w.circles, torch.zeros(2, 3, dtype=torch.float64))
    for bad in (0, -3, 1025):
        with pytest.raises(ValueError, match="n_beams"):
            nav_scan(w.segments, w.circles, torch.zeros(2, 3, dtype=torch.float64), n_beams=bad)
    with pytest.raises(N.NativeError):
        torch.ops.porl_hip.nav_scan(w.segments, w.circles, torch.zeros(2, 3, dtype=torch.float64))
    assert "nav_scan" in O.SCHEMAS
    with pytest.raises(ValueError, match="min_range"):
        LidarNavSim(w, 4, dt=1.0)                                                  # 0.15 m per step: could pass a wall
    with pytest.raises(ValueError, match="pi"):
        LidarNavSim(w, 4, max_ang_vel=16.0)                                        # more than half a turn per step
    with pytest.raises(TypeError, match="unknown parameter"):
        LidarNavSim(w, 4, gravity=9.81)
    with pytest.raises(ValueError, match="primitives"):
        NavWorld(np.zeros((2049, 4), np.float32))
    from porl_amd.env import beam_table
    assert np.array_equal(beam_table(360), NC.beam_table(360)) and np.array_equal(beam_table(37), NC.beam_table(37))
    import sys
    import porl_amd.env.gazebo  # noqa: F401
    import porl_amd.evaluate  # noqa: F401
    assert "gymnasium" not in sys.modules and "rospy" not in sys.modules
