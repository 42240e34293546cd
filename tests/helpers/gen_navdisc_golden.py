"""Writes tests/golden/navdisc_reward.npz from the reference's own env/env.py:

    python tests/helpers/gen_navdisc_golden.py --reference /path/to/reference

The reference is supplied from outside; nothing of its text is kept here, only what its function returns.  ROS, Gazebo, tf,
gymnasium and stable-baselines3 are not needed: the modules env/env.py imports are replaced in `sys.modules` by empty
stand-ins before the import (gen_navsim_golden.stub_modules), and `Env.setReward` is called unbound on a stub object.

navdisc_reward.npz: the unmodified `Env.setReward(state, done, action)` on a grid — heading over [-3.14, 3.14], distance
in [0.2, 3.6], three goal_distance values, all five actions, and the flag combinations (done, get_goalbox) -> reward and
the status the call left.  Data only, a few KB.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from helpers.gen_navsim_golden import Quiet, stub_modules  # noqa: E402

STATUS = {"running": 0, "hit": 1, "goal": 2}


def load_env(reference):
    stub_modules()
    sys.path.insert(0, reference)
    from env.env import Env
    return Env


def gen_reward(Env):
    headings = [round(-3.14 + 6.28 * k / 20, 2) for k in range(21)]
    distances = [0.2, 0.21, 0.37, 1.0, 1.93, 3.6]
    goal_distances = [0.25, 1.3, 3.5]
    flag_sets = [(False, False), (False, True), (True, False), (True, True)]     # 4 and the 5 actions are coprime: all meet
    rec = {k: [] for k in ("heading", "distance", "goal_distance", "action", "done", "goalbox", "reward", "status")}
    k = 0
    for h in headings:
        for d in distances:
            for gd in goal_distances:
                for a in range(5):
                    done, box = flag_sets[k % 4]
                    k += 1
                    e = types.SimpleNamespace(goal_distance=gd, get_goalbox=box, pub_cmd_vel=Quiet(), status="running")
                    state = [0.5] * 360 + [h, d]
                    r = Env.setReward(e, state, done, a)
                    for name, v in (("heading", h), ("distance", d), ("goal_distance", gd), ("action", a), ("done", done),
                                    ("goalbox", box), ("reward", float(r)), ("status", STATUS[e.status])):
                        rec[name].append(v)
    kinds = dict(action=np.int64, status=np.int64, done=np.bool_, goalbox=np.bool_)
    return {name: np.array(v, dtype=kinds.get(name, np.float64)) for name, v in rec.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds env/env.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "golden"))
    a = ap.parse_args()
    out = gen_reward(load_env(a.reference))
    np.savez_compressed(os.path.join(a.out, "navdisc_reward.npz"), **out)
    print("wrote navdisc_reward.npz:", len(out["reward"]), "cases to", a.out)
