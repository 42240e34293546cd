"""Writes tests/golden/navsim_sarsa.npz and tests/golden/navsim_reset.npz from the reference's own env/gazebo.py:

    python tests/helpers/gen_navsim_golden.py --reference /path/to/reference

The reference is supplied from outside; nothing of its text is kept here, only what its functions return.
ROS, Gazebo, tf, gymnasium and stable-baselines3 are not needed: the modules env/gazebo.py imports are replaced in
`sys.modules` by empty stand-ins before the import, and `Env` objects are made without running its constructor.

navsim_sarsa.npz: the unmodified `Env.getSarsa` (through `getRelativeGoal`, `getState`, `lidarPreprocess`) on ~200 cases
of pose, heading, goal, previous distance and angle, and a scan with inf and NaN beams -> state, reward, terminated,
status.
navsim_reset.npz: the unmodified `Env.random_pts_map` with `np.random.randint` / `np.random.uniform` replaced, for the
call, by the simulator's counter stream (tests/helpers/navsim_cases.py: `u01`) -> positions and draws consumed for 256
(seed, env, episode) triples.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from helpers import navsim_cases as NC  # noqa: E402

STATUS = {"running": 0, "hit": 1, "goal": 2}


def stub_modules():
    class Anything:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return Anything()

        def __getattr__(self, name):
            return Anything()

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__getattr__ = lambda attr: Anything          # any other name: a class that accepts everything
        sys.modules[name] = m
        return m

    class GymEnv:
        def __init__(self, *a, **k):
            pass

    for name in ("rospy", "gazebo_msgs", "gazebo_msgs.msg", "gazebo_msgs.srv", "geometry_msgs", "geometry_msgs.msg",
                 "sensor_msgs", "sensor_msgs.msg", "nav_msgs", "nav_msgs.msg", "std_srvs", "std_srvs.srv", "tf",
                 "tf.transformations", "stable_baselines3", "stable_baselines3.common",
                 "stable_baselines3.common.env_checker"):
        module(name)
    module("gymnasium", Env=GymEnv, spaces=module("gymnasium.spaces"))


def load_env(reference):
    stub_modules()
    sys.path.insert(0, reference)
    from env.gazebo import Env
    return Env


class Quiet:
    def publish(self, *a, **k):
        pass


def bare_env(Env, rank=0):
    e = object.__new__(Env)
    e.map_x, e.map_y, e.rank, e.min_range, e.status = -10., -10., rank, 0.13, "running"
    e.pub_cmd_vel = Quiet()
    return e


def gen_sarsa(Env, n=208, seed=0):
    rng = np.random.default_rng(seed)
    rec = {k: [] for k in ("pose", "goal", "prev", "scan", "state", "reward", "terminated", "status")}
    for k in range(n):
        e = bare_env(Env)
        x, y = rng.uniform(-10, -5), rng.uniform(5, 10)
        heading = rng.uniform(-np.pi, np.pi)
        mode = k % 4
        dist = rng.uniform(0.05, 0.19) if mode == 1 else rng.uniform(0.21, 3.5)       # mode 1: inside the goal radius
        th = rng.uniform(-np.pi, np.pi)
        gx, gy = x + dist * np.cos(th), y + dist * np.sin(th)
        prev_d, prev_a = dist + rng.uniform(-0.05, 0.05), rng.uniform(0, np.pi)
        scan = rng.uniform(0.2, 3.5, 360).astype(np.float32)
        scan[rng.random(360) < 0.1] = np.inf
        scan[rng.random(360) < 0.03] = np.nan
        if mode == 2:
            scan[rng.integers(360)] = np.float32(rng.uniform(0.01, 0.129))             # a hit
        if mode == 3 and k % 8 == 3:
            scan[rng.integers(360)] = 0.0                                            # a zero range is no hit
        e.position = types.SimpleNamespace(x=x, y=y)
        e.heading, e.goal_x, e.goal_y, e.goal_distance, e.goal_angle = heading, gx, gy, prev_d, prev_a
        state, reward, terminated = e.getSarsa(types.SimpleNamespace(ranges=[float(v) for v in scan]))
        rec["pose"].append([x, y, heading]), rec["goal"].append([gx, gy]), rec["prev"].append([prev_d, prev_a])
        rec["scan"].append(scan), rec["state"].append(np.asarray(state, np.float64)), rec["reward"].append(float(reward))
        rec["terminated"].append(bool(terminated)), rec["status"].append(STATUS[e.status])
        rec.setdefault("new_prev", []).append([e.goal_distance, e.goal_angle])
    return {k: np.array(v) for k, v in rec.items()}


def gen_reset(Env):
    seeds = [0, 1, 12345, (1 << 63) + 5]
    bases, episodes = [0, 1000], [1, 2, 3, 7, 100, 12345, 1 << 31, 1 << 40]
    rec = {k: [] for k in ("seed", "env", "episode", "xy", "draws")}
    saved = np.random.randint, np.random.uniform
    try:
        for seed in seeds:
            for base in bases:
                for i in range(4):
                    for ep in episodes:
                        key, st = NC.robot_key(seed, base + i), dict(j=0)

                        def randint(n, key=key, ep=ep, st=st):
                            u = NC.u01(key, ep, st["j"])
                            st["j"] += 1
                            return int(np.floor(n * u))

                        def uniform(lo, hi, key=key, ep=ep, st=st):
                            assert lo == 0.16 and abs(hi - 0.84) < 1e-15
                            u = NC.u01(key, ep, st["j"])
                            st["j"] += 1
                            return 0.16 + 0.68 * u

                        np.random.randint, np.random.uniform = randint, uniform
                        x1, y1, x2, y2 = bare_env(Env).random_pts_map()
                        assert st["j"] < NC.MAX_DRAWS
                        rec["seed"].append(seed), rec["env"].append(base + i), rec["episode"].append(ep)
                        rec["xy"].append([x1, y1, x2, y2]), rec["draws"].append(st["j"])
    finally:
        np.random.randint, np.random.uniform = saved
    out = {k: np.array(v, dtype=np.uint64 if k == "seed" else (np.float64 if k == "xy" else np.int64)) for k, v in rec.items()}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds env/gazebo.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "golden"))
    a = ap.parse_args()
    Env = load_env(a.reference)
    np.savez_compressed(os.path.join(a.out, "navsim_sarsa.npz"), **gen_sarsa(Env))
    np.savez_compressed(os.path.join(a.out, "navsim_reset.npz"), **gen_reset(Env))
    print("wrote navsim_sarsa.npz, navsim_reset.npz to", a.out)
