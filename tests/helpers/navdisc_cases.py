"""The discrete lidar navigation task (the reference's env/env.py) in fp64 numpy, in this project's own words: what
csrc/navsim_discrete.hpp runs on the device, on the ray cast, the unicycle step and the reset draw of navsim_cases, plus
the counter stream and rule of porl_qnet_select.  Arithmetic is written operation for operation as the kernel's; only
sin / cos / atan2 / exp2 may differ from it by an ulp of fp64.

Margins: the geometric, threshold and reset margins of navsim_cases, and `margin_round`, the distance of 100 * heading,
100 * distance and 500 * tr from the nearest half on the states actually met (where rint(100 x) / 100 and Python's
decimal-exact round(x, 2) — or two fp64 implementations an ulp apart — could disagree).
"""
import math

import numpy as np

from helpers import navsim_cases as NC

PARAMS = dict(NC.params(no_return=3.5, goal_dist_lo=0.25, hit_reward=-200.0, goal_reward=200.0), lin_vel=0.15, ang_step=0.75)
MARGIN_ROUND = 1e-7
RUNNING, HIT, GOAL, TIMELIMITED = NC.RUNNING, NC.HIT, NC.GOAL, NC.TIMELIMITED


def params(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return p


def round2(x):
    return float(np.rint(100.0 * x)) / 100.0


def half_margin(x):
    """Distance of x from the nearest k + 0.5."""
    return abs((x - 0.5) - float(np.rint(x - 0.5)))


def tail(st):
    """(heading, distance, margin): the rounded observation entries; margin over both roundings and the wrap test."""
    gx, gy = st[3] - st[0], st[4] - st[1]
    h = math.atan2(gy, gx) - st[2]
    wrap = min(abs(h - math.pi), abs(h + math.pi))
    if h > math.pi:
        h -= 2.0 * math.pi
    elif h < -math.pi:
        h += 2.0 * math.pi
    d = math.sqrt(gx * gx + gy * gy)
    return round2(h), round2(d), min(half_margin(100.0 * h), half_margin(100.0 * d)), wrap


def yaw_term(heading, a):
    angle = -math.pi / 4.0 + heading + math.pi / 8.0 * a + math.pi / 2.0
    m = (0.5 * angle) % (2.0 * math.pi)                 # Python's %: non-negative for a positive divisor
    v = 0.25 + m / math.pi
    return 1.0 - 4.0 * abs(0.5 - (v - math.floor(v)))


def shaped_reward(heading, distance, goal_distance, a):
    """(reward, margin of the rounding of 5 tr)."""
    tr5 = yaw_term(heading, a) * 5.0
    return round2(tr5) * 2.0 ** (distance / goal_distance), half_margin(100.0 * tr5)


def reward(heading, distance, goal_distance, a, done, goal, p=PARAMS):
    """setReward: the shaped reward, or goal_reward / hit_reward on a finished step (the goal wins)."""
    if done:
        return p["goal_reward"] if goal else p["hit_reward"]
    return shaped_reward(heading, distance, goal_distance, a)[0]


def command(a, n_actions, p=PARAMS):
    """(clamped index, v, w) of action index a."""
    a = min(max(int(a), 0), n_actions - 1)
    return a, p["lin_vel"], ((n_actions - 1) / 2.0 - a) * p["ang_step"]


class Sim:
    """The device simulator's semantics on the host: same fields, same order of operations."""

    def __init__(self, world, n, n_actions=5, seed=0, env_offset=0, auto_reset=False, p=PARAMS):
        self.seg, self.cir = world
        self.n, self.A, self.seed, self.env_offset, self.auto_reset, self.p = n, n_actions, seed, env_offset, auto_reset, p
        self.S = p["n_beams"] + 2
        self.state = np.zeros((n, 8))
        self.counters = np.zeros((n, 4), np.int64)
        self.counters[:, 2] = TIMELIMITED
        self.obs = np.zeros((n, self.S), np.float32)
        self.tallies = np.zeros((n, 4))
        self.returns = np.zeros(n)
        self.margin_geo = self.margin_thr = self.margin_reset = self.margin_round = math.inf
        self.min_spawn_scan = math.inf

    def _cast(self, poses):
        out, geo, thr = NC.cast(self.seg, self.cir, poses, self.p, with_margin=True)
        self.margin_geo, self.margin_thr = min(self.margin_geo, geo), min(self.margin_thr, thr)
        return out

    def _tail(self, st):
        h, d, rnd, wrap = tail(st)
        self.margin_round, self.margin_thr = min(self.margin_round, rnd), min(self.margin_thr, wrap)
        return h, d

    def _respawn(self, i):
        st, cn = self.state[i], self.counters[i]
        e = int(cn[1]) + 1
        X1, Y1, X2, Y2, j, capped, m = NC.reset_draw(self.seed, self.env_offset + i, e, self.p)
        self.margin_reset = min(self.margin_reset, m)
        st[:7] = X1, Y1, 0.0, X2, Y2, 0.0, 0.0
        h, d = self._tail(st)
        st[7] = d
        cn[:] = 0, e, NC.DRAW_CAP if capped else 0, j
        return h, d

    def _row(self, scan, t):
        return np.concatenate([scan, np.array(t, np.float64).astype(np.float32)])

    def reset(self, mask=None):
        idx = [i for i in range(self.n) if mask is None or mask[i]]
        tails = {i: self._respawn(i) for i in idx}
        if idx:
            scans = self._cast(self.state[idx, :3])
            self.min_spawn_scan = min(self.min_spawn_scan, float(scans.min()))
            for k, i in enumerate(idx):
                self.obs[i] = self._row(scans[k], tails[i])
                self.returns[i] = 0.0
        return self.obs

    def step(self, actions):
        """-> dict(next_obs, reward, flags, status, actions (clamped), ran (robots that stepped), obs_before)."""
        p, n, S = self.p, self.n, self.S
        next_obs = np.zeros((n, S), np.float32)
        reward_ = np.zeros(n, np.float32)
        flags = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        acts = np.zeros(n, np.int64)
        before = self.obs.copy()
        run = [i for i in range(n) if (self.counters[i, 2] & 0xff) == RUNNING]
        for i in range(n):
            if i not in run:
                next_obs[i] = self.obs[i]
                status[i] = self.counters[i, 2]
        for i in run:
            acts[i], v, om = command(actions[i], self.A, p)
            self.state[i, :3] = NC.move(self.state[i], v, om, p)
        respawned = []
        if run:
            scans = self._cast(self.state[run, :3])
        for k, i in enumerate(run):
            st, cn = self.state[i], self.counters[i]
            h, d = self._tail(st)
            mn = float(scans[k].astype(np.float64).min())
            self.margin_thr = min(self.margin_thr, abs(mn - p["min_range"]))
            hit = 0.0 < mn < p["min_range"]
            goal = d < p["goal_radius"]
            term = hit or goal
            r, rnd = shaped_reward(h, d, st[7], int(acts[i]))
            stat = RUNNING
            if term:
                r, stat = (p["goal_reward"], GOAL) if goal else (p["hit_reward"], HIT)
            else:
                self.margin_round = min(self.margin_round, rnd)
            cn[0] += 1
            trunc = cn[0] >= p["episode_step"]
            if trunc:
                stat = TIMELIMITED
            rf = np.float32(r)
            o = self._row(scans[k], (h, d))
            next_obs[i], reward_[i], flags[i], status[i] = o, rf, int(term) | (int(trunc) << 1), stat
            ret = self.returns[i] + float(rf)
            if term or trunc:
                self.tallies[i] += (1.0, ret, 1.0 if goal else 0.0, 1.0 if hit and not goal else 0.0)
                self.returns[i] = 0.0
            else:
                self.returns[i] = ret
            if (term or trunc) and self.auto_reset:
                respawned.append((i, self._respawn(i)))
            else:
                cn[2] = stat
                self.obs[i] = o
        if respawned:
            idx = [i for i, _ in respawned]
            scans = self._cast(self.state[idx, :3])
            self.min_spawn_scan = min(self.min_spawn_scan, float(scans.min()))
            for k, (i, t) in enumerate(respawned):
                self.obs[i] = self._row(scans[k], t)
        ran = np.zeros(n, bool)
        ran[run] = True
        return dict(next_obs=next_obs, reward=reward_, flags=flags, status=status, actions=acts, ran=ran, obs_before=before)

    def margins(self):
        """(geometric, thresholds, reset rejections, roundings): smallest distance of any decision met so far from its tie."""
        return self.margin_geo, self.margin_thr, self.margin_reset, self.margin_round


# ---- the roll-out the GPU tests repeat ----------------------------------------------------------------------------------
ROLLOUT = dict(n=24, T=40, episode_step=25, n_actions=5, seed=9)


def steer_action(obs, n_actions, n_beams, p=PARAMS):
    """The action whose angular velocity is nearest to 2 * heading (the observation's rounded heading), fp64."""
    w = np.clip(2.0 * obs[..., n_beams].astype(np.float64), -1.5, 1.5)
    if p["ang_step"] == 0.0:
        return np.zeros(w.shape, np.int64)
    a = np.rint((n_actions - 1) / 2.0 - w / p["ang_step"])
    return np.clip(a, 0, n_actions - 1).astype(np.int64)


def rollout_actions(obs, t, seed, n_actions=5, n_beams=360, p=PARAMS):
    """Actions of the roll-out at step t: every third robot steers at the goal, the others draw uniform indices from a
    generator keyed by (seed, t) alone, so they do not depend on what the robots see."""
    a = steer_action(obs, n_actions, n_beams, p)
    rnd = np.random.default_rng([seed, t]).integers(0, n_actions, obs.shape[0])
    sel = np.arange(obs.shape[0]) % 3 != 0
    a[sel] = rnd[sel]
    return a


def rollout(**over):
    """-> (sim, outcome counts): the host roll-out with ROLLOUT's settings (auto_reset)."""
    cfg = dict(ROLLOUT)
    cfg.update(over)
    p = params(episode_step=cfg["episode_step"], **({"n_beams": cfg["n_beams"]} if "n_beams" in cfg else {}))
    sim = Sim(NC.lattice(), cfg["n"], cfg["n_actions"], seed=cfg["seed"], auto_reset=True, p=p)
    sim.reset()
    counts = {HIT: 0, GOAL: 0, TIMELIMITED: 0}
    for t in range(cfg["T"]):
        out = sim.step(rollout_actions(sim.obs, t, cfg["seed"], cfg["n_actions"], p["n_beams"], p))
        term, trunc = (out["flags"] & 1) != 0, (out["flags"] & 2) != 0
        counts[TIMELIMITED] += int((trunc & ~term).sum())
    counts[GOAL], counts[HIT] = int(sim.tallies[:, 2].sum()), int(sim.tallies[:, 3].sum())
    return sim, counts


# ---- porl_qnet_select ---------------------------------------------------------------------------------------------------
def select(q, epsilon, seed, t, env_offset=0):
    """Epsilon-greedy over q (n, A) float32: robot i draws u1, u2 = draws 0, 1 of "episode" t of its counter stream."""
    q = np.asarray(q, np.float32)
    n, A = q.shape
    out = np.zeros(n, np.int64)
    for i in range(n):
        key = NC.robot_key(seed, env_offset + i)
        if NC.u01(key, t, 0) < epsilon:
            out[i] = min(int(math.floor(A * NC.u01(key, t, 1))), A - 1)
        else:
            best, pick = q[i, 0], 0
            for j in range(1, A):
                v = q[i, j]
                if best == best and (v > best or v != v):
                    best, pick = v, j
            out[i] = pick
    return out
