"""The discrete lidar navigation task without a GPU: the numpy restatement (tests/helpers/navdisc_cases.py) against what
the reference's own `Env.setReward` returned (tests/golden/navdisc_reward.npz, written by
tests/helpers/gen_navdisc_golden.py), the roll-out the GPU tests repeat, every rejected argument of the four new entry
points (through ctypes: the library loads without a GPU and judges its arguments before any device call), the agreement
of header, exported symbols and ctypes table, and the Python layer's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from helpers import navdisc_cases as DC
from helpers import navsim_cases as NC
from porl_amd import _native as N

ENTRY_POINTS = ("porl_nav_dreset", "porl_nav_dstep", "porl_qnet_select", "porl_qnet_act_rows")


def test_abi_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(", txt), name
        assert name in N.SYMBOLS
        assert hasattr(N.lib(), name)
        assert getattr(N.lib(), name).argtypes is not None                          # declared in the ctypes table
    assert re.search(r"#define\s+PORL_ABI_VERSION\s+12\b", txt)                    # additions only
    assert N.ABI_VERSION == 12 and N.lib().porl_abi_version() == 12
    # the ctypes mirrors have the header's fields in the header's order, and porl_nav_params kept its layout
    body = txt.split("typedef struct porl_nav_discrete {")[1].split("} porl_nav_discrete;")[0]
    fields = re.findall(r"^\s*(?:double|int32_t)\s+(\w+);", body, re.M)
    assert fields == [f[0] for f in N.NavDiscrete._fields_] == ["n_actions", "lin_vel", "ang_step", "goal_reward", "hit_reward"]
    assert C.sizeof(N.NavDiscrete) == 40 and N.NavDiscrete.lin_vel.offset == 8
    assert C.sizeof(N.NavParams) == 16 * 8 + 6 * 4
    # argument counts of the declarations and of the ctypes table agree
    for name in ENTRY_POINTS:
        decl = re.search(rf"\bint\s+{name}\s*\(([^;]*?)\)\s*;", txt, re.S).group(1)
        assert len(decl.split(",")) == len(getattr(N.lib(), name).argtypes), name


# ---- the restatement against the reference's recorded results -------------------------------------------------------------
def test_reward_matches_the_reference_exactly():
    z, _ = load_golden("navdisc_reward")
    n = len(z["reward"])
    assert 1800 <= n <= 2200
    assert set(np.unique(z["action"])) == set(range(5)) and len(np.unique(z["goal_distance"])) == 3
    assert z["heading"].min() == -3.14 and z["heading"].max() == 3.14 and z["distance"].min() == 0.2 and z["distance"].max() == 3.6
    assert {(bool(d), bool(g)) for d, g in zip(z["done"], z["goalbox"])} == {(False, False), (False, True), (True, False), (True, True)}
    worst = np.inf
    for k in range(n):
        h, d, gd, a = float(z["heading"][k]), float(z["distance"][k]), float(z["goal_distance"][k]), int(z["action"][k])
        done, box = bool(z["done"][k]), bool(z["goalbox"][k])
        r = DC.reward(h, d, gd, a, done, box)
        assert r == float(z["reward"][k]), (k, r, z["reward"][k])                   # exactly
        assert int(z["status"][k]) == ((DC.GOAL if box else DC.HIT) if done else DC.RUNNING)
        worst = min(worst, DC.shaped_reward(h, d, gd, a)[1])
    print("smallest margin of 500 tr from a half on the golden grid:", worst)
    assert worst > DC.MARGIN_ROUND                                                 # round(x, 2) and rint(100 x) / 100 cannot differ
    assert (np.abs(z["reward"][~z["done"]]) > 100).any()                           # the 2 ** (d / gd) factor at work


def test_yaw_term_closed_forms():
    # facing the goal, the middle action scores 1; the term is 2-periodic in angle / pi and lies in [-1, 1]
    assert abs(DC.yaw_term(0.0, 2) - 1.0) < 1e-12
    assert abs(DC.yaw_term(0.0, 0) - DC.yaw_term(0.0, 4)) < 1e-12                  # symmetric about the middle action
    for h in np.linspace(-3.14, 3.14, 41):
        for a in range(5):
            assert -1.0 - 1e-12 <= DC.yaw_term(h, a) <= 1.0 + 1e-12
    assert DC.command(-3, 5) == (0, 0.15, 1.5) and DC.command(99, 5) == (4, 0.15, -1.5) and DC.command(2, 5)[2] == 0.0
    assert DC.command(1, 3) == (1, 0.15, 0.0) and DC.command(0, 1) == (0, 0.15, 0.0)
    assert DC.round2(0.125) == 0.12 and DC.round2(1.234) == 1.23 and DC.round2(-0.456) == -0.46   # rint(100 x) / 100
    # the stated deviation: 100 * 2.675 rounds to 267.5 in fp64, a tie, where Python's decimal-exact round sees 2.67499..
    assert DC.round2(2.675) == 2.68 and round(2.675, 2) == 2.67 and DC.half_margin(100.0 * 2.675) == 0.0
    assert DC.half_margin(12.5) == 0.0 and abs(DC.half_margin(12.75) - 0.25) < 1e-15


def test_rollout_on_the_host():
    """The roll-out the GPU test repeats (24 robots, 40 steps, episodes of 25 steps, seed 9): every outcome occurs at
    least twice and no decision lies near a tie.  Measured with this restatement: 14 hits, 3 goals, 20 step limits;
    smallest margins geometric 1.18e-07, thresholds 1.10e-06, reset rejections 6.42e-04, roundings (100 heading, 100
    distance, 500 tr from a half) 3.53e-04; smallest scan at a spawn 0.1606."""
    sim, counts = DC.rollout()
    geo, thr, rst, rnd = sim.margins()
    print(counts, geo, thr, rst, rnd, sim.min_spawn_scan)
    assert counts == {DC.HIT: 14, DC.GOAL: 3, DC.TIMELIMITED: 20}
    assert min(counts.values()) >= 2
    assert min(geo, thr, rst) > NC.MARGIN
    assert rnd > DC.MARGIN_ROUND
    assert sim.min_spawn_scan >= 0.13
    assert not (sim.counters[:, 2] & NC.DRAW_CAP).any() and sim.counters[:, 3].max() <= 64
    assert sim.tallies[:, 0].sum() == sum(counts.values())
    # goal_distance is the rounded distance at reset, within the reference's goal band
    assert (sim.state[:, 7] >= 0.25).all() and (sim.state[:, 7] <= 3.5).all()
    assert np.array_equal(sim.state[:, 7], np.rint(sim.state[:, 7] * 100) / 100)


def test_short_variants_keep_their_margins():
    """The two 5-step variants of the GPU test: 37 beams (less than one wave), and three actions."""
    for over in (dict(n_beams=37), dict(n_actions=3)):
        sim, _ = DC.rollout(T=5, **over)
        geo, thr, rst, rnd = sim.margins()
        print(over, geo, thr, rst, rnd)
        assert min(geo, thr, rst) > NC.MARGIN and rnd > DC.MARGIN_ROUND


def test_select_restatement():
    q = np.array([[1, 3, 3, 2], [np.nan, 5, 1, 0], [0, 1, np.nan, np.nan], [2, 2, 2, 2]], np.float32)
    assert DC.select(q, 0.0, 1, 0).tolist() == [1, 0, 2, 0]                        # ties to the lowest index, NaN is the maximum
    a = DC.select(np.zeros((400, 5), np.float32), 1.0, 7, 3)
    assert set(a.tolist()) == set(range(5))                                        # exploring covers every action
    both = DC.select(np.zeros((64, 5), np.float32), 1.0, 7, 3)
    assert np.array_equal(both[32:], DC.select(np.zeros((32, 5), np.float32), 1.0, 7, 3, env_offset=32))
    assert not np.array_equal(DC.select(np.zeros((64, 5), np.float32), 1.0, 7, 4), both)      # the act-step keys the draw


# ---- rejected arguments ---------------------------------------------------------------------------------------------------
_F = (C.c_float * 4096)()
_G = (C.c_float * 4096)()
_D = (C.c_double * 4096)()
_I = (C.c_int64 * 64)()


def _params(**over):
    p = {k: v for k, v in DC.PARAMS.items() if k not in ("lin_vel", "ang_step")}
    p.update(over)
    return N.NavParams(**p)


def _task(**over):
    t = dict(n_actions=5, lin_vel=0.15, ang_step=0.75, goal_reward=200.0, hit_reward=-200.0)
    t.update(over)
    return N.NavDiscrete(**t)


def _mirror(capacity=64, **over):
    m = dict(states=C.addressof(_D), next_states=C.addressof(_D) + 8192, actions=C.addressof(_I), rewards=C.addressof(_G),
             dones=C.addressof(_G) + 1024)
    m.update(over)
    return N.QnetMirror(m["states"], m["next_states"], m["actions"], m["rewards"], m["dones"], capacity)


def _dstep(**over):
    a = dict(M=4, Cn=16, params=_params(), task=_task(), env_offset=0, actions=_I, state=_D, counters=_I, obs=_F,
             obs_stride=362, next_obs=_G, next_stride=362, reward=_F, flags=_I, status=_I, replay=None, base=0, tallies=None,
             returns=None, n=4)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_nav_dstep(_F, a["M"], _F, a["Cn"], _D, a["params"], a["task"], 1, a["env_offset"], a["actions"], a["state"],
                            a["counters"], a["obs"], a["obs_stride"], a["next_obs"], a["next_stride"], a["reward"], a["flags"],
                            a["status"], a["replay"], a["base"], a["tallies"], a["returns"], a["n"], None)
    return rc, lib.porl_last_error().decode()


def _dreset(**over):
    a = dict(params=_params(), task=_task(), state=_D, counters=_I, obs=_F, obs_stride=362, n=4)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_nav_dreset(_F, 4, _F, 16, _D, a["params"], a["task"], 1, 0, None, a["state"], a["counters"], a["obs"],
                             a["obs_stride"], None, a["n"], None)
    return rc, lib.porl_last_error().decode()


def _select(**over):
    a = dict(q=_F, q_rs=5, A=5, n=8, eps=0.1, env_offset=0, t=0, out=_I)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_qnet_select(a["q"], a["q_rs"], a["A"], a["n"], a["eps"], 1, a["env_offset"], a["t"], a["out"], None)
    return rc, lib.porl_last_error().decode()


@pytest.mark.parametrize("fn,over,word", [
    (_dstep, dict(actions=None), "null actions"), (_dstep, dict(state=None), "null state"), (_dstep, dict(flags=None), "null flags"),
    (_dstep, dict(task=None), "null task"), (_dstep, dict(params=None), "null params"), (_dstep, dict(n=0), "n 0"),
    (_dstep, dict(task=_task(n_actions=0)), "n_actions 0"), (_dstep, dict(task=_task(n_actions=6)), "n_actions 6"),
    (_dstep, dict(obs_stride=361), "obs_stride"), (_dstep, dict(next_stride=361), "next_stride"),
    (_dstep, dict(next_obs=_F), "next_obs must not be obs"),
    (_dstep, dict(M=2040, Cn=9), "primitives"), (_dstep, dict(params=_params(n_beams=1025)), "n_beams"),
    (_dstep, dict(params=_params(n_beams=0)), "n_beams"), (_dstep, dict(params=_params(layout=1)), "obs_stride"),
    (_dstep, dict(params=_params(layout=1), obs_stride=365), "PORL_NAV_LAYOUT_GOAL"),
    (_dstep, dict(task=_task(lin_vel=0.7)), "min_range"), (_dstep, dict(task=_task(lin_vel=float("nan"))), "lin_vel"),
    (_dstep, dict(task=_task(ang_step=9.0)), "below pi"), (_dstep, dict(task=_task(goal_reward=float("inf"))), "goal_reward"),
    (_dstep, dict(replay=C.pointer(_mirror(capacity=3))), "share a slot"),
    (_dstep, dict(replay=C.pointer(_mirror(rewards=None))), "null replay array"),
    (_dstep, dict(replay=C.pointer(_mirror()), base=64), "replay_base"), (_dstep, dict(replay=C.pointer(_mirror()), base=-1), "replay_base"),
    (_dstep, dict(base=5), "without a replay"), (_dstep, dict(tallies=_D), "tallies and returns"),
    (_dstep, dict(env_offset=-1), "env_offset"),
    (_dreset, dict(task=_task(n_actions=6)), "n_actions 6"), (_dreset, dict(obs=None), "null obs"), (_dreset, dict(n=0), "n 0"),
    (_dreset, dict(params=_params(n_beams=1025)), "n_beams"), (_dreset, dict(obs_stride=361), "obs_stride"),
    (_select, dict(q=None), "null action values"), (_select, dict(out=None), "null out"), (_select, dict(n=0), "n 0"),
    (_select, dict(A=0), "n_actions 0"), (_select, dict(A=65, q_rs=65), "n_actions 65"), (_select, dict(q_rs=4), "q_rs"),
    (_select, dict(eps=-0.01), "epsilon"), (_select, dict(eps=1.01), "epsilon"), (_select, dict(eps=float("nan")), "epsilon"),
    (_select, dict(eps=float("inf")), "epsilon"), (_select, dict(env_offset=-1), "env_offset"),
])
def test_bad_arguments_are_rejected_by_name(fn, over, word):
    rc, msg = fn(**over)
    assert rc == -1 and word in msg, (rc, msg)


def test_act_rows_rejects_before_any_launch():
    lib = N.lib()
    assert lib.porl_qnet_act_rows(None, 0, _F, 8, 4, _G, 5, 0.1, 1, 0, 0, _I, None) == -1
    assert "null engine" in lib.porl_last_error().decode()
    cfg = N.QnetCfg(8, 5, 2, (C.c_int32 * 8)(64, 64), 32)
    h = C.c_void_p()
    assert lib.porl_qnet_create(C.byref(cfg), C.byref(h)) == 0
    try:
        rc = lib.porl_qnet_act_rows(h, 0, _F, 8, 4, _G, 5, 0.1, 1, 0, 0, _I, None)
        assert rc != 0 and "porl_qnet_bind" in lib.porl_last_error().decode()      # an unbound engine launches nothing
    finally:
        lib.porl_qnet_destroy(h)


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def test_python_surface_has_no_cpu_path():
    import torch
    from porl_amd.buffer.device_replay import DeviceReplay
    from porl_amd.env import DiscreteLidarNavSim, Env, NavWorld
    from porl_amd.env import env as E
    w = NavWorld.lattice()
    assert E.DEFAULTS["no_return"] == 3.5 and E.DEFAULTS["goal_dist_lo"] == 0.25 and E.DEFAULTS["goal_reward"] == 200.0
    for bad in (0, 6, -1):
        with pytest.raises(ValueError, match="n_actions"):
            DiscreteLidarNavSim(w, 4, n_actions=bad)
    with pytest.raises(ValueError, match="n_actions"):
        Env(6, 362)
    with pytest.raises(N.NativeError, match="no CPU path"):
        DiscreteLidarNavSim(w, 4, device="cpu")
    with pytest.raises(N.NativeError, match="no CPU path"):
        DeviceReplay(16, 362, device="cpu")
    with pytest.raises(TypeError, match="unknown parameter"):
        DiscreteLidarNavSim(w, 4, gravity=9.81)
    with pytest.raises(ValueError, match="min_range"):
        DiscreteLidarNavSim(w, 4, lin_vel=0.7)
    with pytest.raises(ValueError, match="n_beams"):
        DiscreteLidarNavSim(w, 4, n_beams=1025)
    from porl_amd.train.cql_trainer import CQLTrainer
    from porl_amd.train.vector_online import train_vectorized  # noqa: F401
    assert callable(CQLTrainer.train_vectorized)
    import sys
    assert "gymnasium" not in sys.modules and "rospy" not in sys.modules
    assert torch is not None


def test_family_table_takes_each_trainer_class_once():
    """train/vector_online.py's table on the classes alone (PER and IQN trainers need a device to exist): PER and BCQ
    subclass CQLTrainer and must be found before plain Q; a subclass stays in its base's family."""
    from porl_amd.train import vector_online as VO
    from porl_amd.train.bcq_trainer import BCQTrainer
    from porl_amd.train.c51_trainer import C51Trainer
    from porl_amd.train.cql_trainer import CQLTrainer
    from porl_amd.train.dddqn_trainer import DDDQNTrainer
    from porl_amd.train.dist_trainer import DistTrainerBase
    from porl_amd.train.dqn_per_trainer import PERTrainer
    from porl_amd.train.dqn_trainer import DDQNTrainer, DQNTrainer
    from porl_amd.train.iqn_trainer import IQNTrainer
    from porl_amd.train.qr_dqn_trainer import QRDQNTrainer
    from porl_amd.train.vector_offline import batched_act
    assert issubclass(PERTrainer, CQLTrainer) and issubclass(BCQTrainer, CQLTrainer)
    want = {VO.PLAIN: (CQLTrainer, DQNTrainer, DDQNTrainer, DDDQNTrainer), VO.PER: (PERTrainer,), VO.BCQ: (BCQTrainer,),
            VO.DIST: (DistTrainerBase, C51Trainer, QRDQNTrainer), VO.IQN: (IQNTrainer,)}
    assert set(want) == set(VO.FAMILIES) and len(VO.FAMILIES) == 5
    for fam, classes in want.items():
        for cls in classes:
            assert VO.family_of(cls) is fam, cls.__name__
            assert VO.family_of(type("Sub", (cls,), {})) is fam, cls.__name__
    assert VO.family_of(object) is None and VO.family_of(type(None)) is None
    # every family with a loop names it and has a learn step; BCQ has an act call only
    loops = {fam.loop: fam for fam in VO.FAMILIES if fam.loop}
    assert sorted(loops) == ["train_vectorized", "train_vectorized_dist", "train_vectorized_iqn", "train_vectorized_per"]
    assert all(callable(fam.learn) and callable(getattr(VO, name)) for name, fam in loops.items())
    assert VO.BCQ.loop is None and VO.BCQ.learn is None and all(callable(fam.act) for fam in VO.FAMILIES)
    with pytest.raises(NotImplementedError, match="object has no batched act call in the discrete task"):
        batched_act(object(), 8)
