"""The lidar navigation task in fp64 numpy, in this project's own words: the ray cast, the unicycle step, the reward and
termination rules and the start / goal draw that csrc/navsim.hpp runs on the device, plus `margins`, the distance of
every discontinuous decision from its tie.  Tests compare the device per element against this file on cases whose margins
exceed MARGIN, so two correct fp64 implementations cannot disagree on a decision.

Arithmetic is written operation for operation as the kernel's (which compiles without fused multiply-adds): products,
sums, quotients and square roots agree bit for bit; only sin / cos / atan2 may differ by an ulp of fp64.
"""
import math

import numpy as np

MARGIN = 1e-9
M64 = (1 << 64) - 1
PARAMS = dict(dt=0.2, max_lin_vel=0.15, max_ang_vel=1.5, min_range=0.13, range_max=3.5, no_return=10.0, goal_radius=0.2,
              hit_reward=-500.0, goal_reward=500.0, origin_x=-10.0, origin_y=5.0, spawn_lo=0.16, spawn_span=0.68,
              min_gap_sq=0.01, goal_dist_lo=0.3, goal_dist_hi=3.5, n_beams=360, episode_step=500, cells=5)
MAX_DRAWS = 256
RUNNING, HIT, GOAL, TIMELIMITED, DRAW_CAP = 0, 1, 2, 3, 256


def params(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return p


# ---- the counter stream -------------------------------------------------------------------------------------------------
def sm64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def robot_key(seed, env):
    return sm64((seed & M64) ^ sm64(env & M64))


def u01(key, episode, j):
    return float(sm64(key ^ sm64((256 * episode + j) & M64)) >> 11) * 2.0 ** -53


def reset_draw(seed, env, episode, p=PARAMS):
    """(x1, y1, x2, y2, draws_used, capped, margin): the start and goal of `episode` of robot `env`; margin = the smallest
    distance of a rejection test from its tie."""
    key = robot_key(seed, env)
    st = dict(j=0, capped=False, margin=math.inf)

    def coord(cur):
        if st["j"] + 2 > MAX_DRAWS:
            st["capped"] = True
            return cur
        k = math.floor(p["cells"] * u01(key, episode, st["j"]))
        f = p["spawn_lo"] + p["spawn_span"] * u01(key, episode, st["j"] + 1)
        st["j"] += 2
        return k + f

    def below(v, bound):
        st["margin"] = min(st["margin"], abs(v - bound))
        return v < bound

    x1 = x2 = y1 = y2 = 0.0
    while below((x1 - x2) * (x1 - x2), p["min_gap_sq"]) and not st["capped"]:
        x1 = coord(x1)
        x2 = coord(x2)
    while below((y1 - y2) * (y1 - y2), p["min_gap_sq"]) and not st["capped"]:
        y1 = coord(y1)
        y2 = coord(y2)
    X1, Y1 = p["origin_x"] + x1, p["origin_y"] + y1
    X2, Y2 = p["origin_x"] + x2, p["origin_y"] + y2

    def far():
        d = math.sqrt((Y2 - Y1) * (Y2 - Y1) + (X2 - X1) * (X2 - X1))
        lo = below(d, p["goal_dist_lo"])
        hi = below(p["goal_dist_hi"], d)
        return lo or hi

    while far() and not st["capped"]:
        x2 = coord(x2)
        y2 = coord(y2)
        X2, Y2 = p["origin_x"] + x2, p["origin_y"] + y2
    return X1, Y1, X2, Y2, st["j"], st["capped"], st["margin"]


# ---- worlds -------------------------------------------------------------------------------------------------------------
def lattice(rank=0, pillar_radius=0.08, map_x=-10.0, map_y=-10.0, cells=5):
    ox, oy = map_x + (rank % 4) * cells, map_y + (3 - rank // 4) * cells
    L = float(cells)
    seg = np.array([[ox, oy, ox + L, oy], [ox + L, oy, ox + L, oy + L], [ox + L, oy + L, ox, oy + L], [ox, oy + L, ox, oy]],
                   np.float32)
    cir = np.array([[ox + i, oy + j, pillar_radius] for j in range(1, cells) for i in range(1, cells)], np.float32)
    return seg, cir


def oblique(seed=3):
    """A custom world with nothing axis-aligned: a tilted quadrilateral of walls, slanted inner walls, pillars of mixed
    radii.  Poses for it: `oblique_poses`."""
    rng = np.random.default_rng(seed)
    c, s = math.cos(0.37), math.sin(0.37)
    corners = np.array([[-3.1, -2.7], [3.3, -2.9], [2.8, 3.2], [-2.9, 2.6]]) @ np.array([[c, s], [-s, c]])
    seg = [np.concatenate([corners[k], corners[(k + 1) % 4]]) for k in range(4)]
    for _ in range(9):
        a = rng.uniform(-2.2, 2.2, 2)
        th = rng.uniform(0, 2 * math.pi)
        L = rng.uniform(0.3, 1.2)
        seg.append(np.concatenate([a, a + L * np.array([math.cos(th), math.sin(th)])]))
    cir = np.column_stack([rng.uniform(-2.3, 2.3, (11, 2)), rng.uniform(0.05, 0.3, 11)])
    return np.array(seg, np.float32), cir.astype(np.float32)


def beam_table(n_beams):
    if n_beams == 360:
        ang = [i * np.pi / 180 for i in range(360)]
    else:
        ang = [2 * np.pi * i / n_beams for i in range(n_beams)]
    return np.array([[np.cos(a), np.sin(a)] for a in ang], dtype=np.float64)


# ---- the ray cast -------------------------------------------------------------------------------------------------------
def cast(segments, circles, poses, p=PARAMS, with_margin=False):
    """Ranges (n, n_beams) as float32, from poses (n, 3) fp64; with_margin also the smallest geometric margin and the
    smallest |t - range_max| of a valid candidate."""
    seg = np.asarray(segments, np.float32).reshape(-1, 4).astype(np.float64)
    cir = np.asarray(circles, np.float32).reshape(-1, 3).astype(np.float64)
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    tab = beam_table(p["n_beams"])
    rm = p["range_max"]
    px, py = poses[:, 0][:, None, None], poses[:, 1][:, None, None]
    cy, sy = np.cos(poses[:, 2])[:, None], np.sin(poses[:, 2])[:, None]
    c, s = tab[:, 0][None, :], tab[:, 1][None, :]
    dx, dy = (c * cy - s * sy)[:, :, None], (s * cy + c * sy)[:, :, None]
    best = np.full(dx.shape[:2], rm)
    geo = thr = math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        if len(seg):
            ax, ay = seg[:, 0], seg[:, 1]
            ex, ey = seg[:, 2] - ax, seg[:, 3] - ay
            wx, wy = ax - px, ay - py
            den = dx * ey - dy * ex
            t = (wx * ey - wy * ex) / den
            sp = (wx * dy - wy * dx) / den
            ok = (den != 0.0) & (sp >= 0.0) & (sp <= 1.0) & (t > 0.0) & (t < rm)
            best = np.minimum(best, np.where(ok, t, rm).min(axis=2))
            if with_margin:
                near = (t > -1e-6) & (t < rm + 1e-6)          # den == 0 gives inf / nan: parallel, no candidate
                if near.any():
                    geo = min(geo, np.abs(den[near]).min(), np.abs(sp[near]).min(), np.abs(sp[near] - 1.0).min())
                hit = (den != 0.0) & (sp >= 0.0) & (sp <= 1.0) & (t > 0.0)
                if hit.any():
                    thr = min(thr, np.abs(t[hit] - rm).min(), np.abs(t[hit]).min())
        if len(cir):
            fx, fy, r = px - cir[:, 0], py - cir[:, 1], cir[:, 2]
            b = -(fx * dx + fy * dy)
            cc = (fx * fx + fy * fy) - r * r
            disc = b * b - cc
            t = b - np.sqrt(np.maximum(disc, 0.0))
            ok = (disc >= 0.0) & (t > 0.0) & (t < rm)
            best = np.minimum(best, np.where(ok, t, rm).min(axis=2))
            if with_margin:
                near = (t > -1e-6) & (t < rm + 1e-6)
                if near.any():
                    geo = min(geo, np.abs(disc[near]).min())
                hit = (disc >= 0.0) & (t > 0.0)
                if hit.any():
                    thr = min(thr, np.abs(t[hit] - rm).min(), np.abs(t[hit]).min())
    out = np.where(best < rm, best.astype(np.float32), np.float32(p["no_return"])).astype(np.float32)
    return (out, float(geo), float(thr)) if with_margin else out


# ---- the task -----------------------------------------------------------------------------------------------------------
def relative_goal(st):
    gx, gy = st[3] - st[0], st[4] - st[1]
    s, c = math.sin(st[2]), math.cos(st[2])
    d = math.sqrt(gx * gx + gy * gy)
    rx, ry = c * gx + s * gy, -s * gx + c * gy
    return d, abs(math.atan2(ry, rx)), rx, ry


def obs_row(scan, st, rx, ry, layout):
    tail = [st[0], st[1], st[2], st[3], st[4]] if layout == "pose" else [rx, ry]
    return np.concatenate([scan, np.array(tail, np.float64).astype(np.float32)])


def clip_command(a, p=PARAMS):
    v, om = float(a[0]), float(a[1])
    v = 0.0 if not math.isfinite(v) else v
    om = 0.0 if not math.isfinite(om) else om
    return min(max(v, 0.0), p["max_lin_vel"]), min(max(om, -p["max_ang_vel"]), p["max_ang_vel"])


def move(st, v, om, p=PARAMS):
    th = om * p["dt"]
    h = th / 2.0
    sinc = math.sin(h) / h if abs(h) >= 1e-4 else 1.0 - h * h / 6.0
    chord = v * p["dt"] * sinc
    x = st[0] + chord * math.cos(st[2] + h)
    y = st[1] + chord * math.sin(st[2] + h)
    yaw = st[2] + th
    if yaw > math.pi:
        yaw -= 2.0 * math.pi
    elif yaw <= -math.pi:
        yaw += 2.0 * math.pi
    return x, y, yaw


def sarsa(st, scan, p=PARAMS):
    """getSarsa on state `st` (updated in place: prev_goal_distance, prev_goal_angle) and the ranges of the scan at its
    pose -> (goal in the robot frame rx, ry, reward, terminated, status, threshold margin).  Non-finite ranges read
    `no_return`."""
    scan = np.asarray(scan, np.float64)
    scan = np.where(np.isfinite(scan), scan, p["no_return"])
    d, ang, rx, ry = relative_goal(st)
    r = st[5] - d if d < st[5] else 2.0 * (st[5] - d)
    r += st[6] - ang if ang < st[6] else 2.0 * (st[6] - ang)
    st[5], st[6] = d, ang
    mn = float(scan.min())
    term, stat = False, RUNNING
    thr = min(abs(mn - p["min_range"]), abs(d - p["goal_radius"]))
    if 0.0 < mn < p["min_range"]:
        term, r, stat = True, p["hit_reward"], HIT
    if d < p["goal_radius"]:
        term, r, stat = True, p["goal_reward"], GOAL
    return rx, ry, r, term, stat, thr


class Sim:
    """The device simulator's semantics on the host: same fields, same order of operations."""

    def __init__(self, world, n, seed=0, env_offset=0, layout="goal", auto_reset=False, p=PARAMS):
        self.seg, self.cir = world
        self.n, self.seed, self.env_offset, self.layout, self.auto_reset, self.p = n, seed, env_offset, layout, auto_reset, p
        self.S = p["n_beams"] + (5 if layout == "pose" else 2)
        self.state = np.zeros((n, 8))
        self.counters = np.zeros((n, 4), np.int64)
        self.counters[:, 2] = TIMELIMITED
        self.obs = np.zeros((n, self.S), np.float32)
        self.margin_geo = self.margin_thr = self.margin_reset = math.inf
        self.min_spawn_scan = math.inf

    def _cast(self, poses):
        out, geo, thr = cast(self.seg, self.cir, poses, self.p, with_margin=True)
        self.margin_geo, self.margin_thr = min(self.margin_geo, geo), min(self.margin_thr, thr)
        return out

    def _respawn(self, i):
        """state, counters of robot i for its next episode; the observation needs a cast at the new pose."""
        st, cn = self.state[i], self.counters[i]
        e = int(cn[1]) + 1
        X1, Y1, X2, Y2, j, capped, m = reset_draw(self.seed, self.env_offset + i, e, self.p)
        self.margin_reset = min(self.margin_reset, m)
        st[:5] = X1, Y1, 0.0, X2, Y2
        d, ang, rx, ry = relative_goal(st)
        st[5], st[6], st[7] = d, ang, 0.0
        cn[:] = 0, e, DRAW_CAP if capped else 0, j
        return rx, ry

    def reset(self, mask=None):
        idx = [i for i in range(self.n) if mask is None or mask[i]]
        tails = {i: self._respawn(i) for i in idx}
        if idx:
            scans = self._cast(self.state[idx, :3])
            self.min_spawn_scan = min(self.min_spawn_scan, float(scans.min()))
            for k, i in enumerate(idx):
                self.obs[i] = obs_row(scans[k], self.state[i], *tails[i], self.layout)
        return self.obs

    def step(self, actions, want_rows=False):
        p, n, S = self.p, self.n, self.S
        next_obs = np.zeros((n, S), np.float32)
        reward = np.zeros(n, np.float32)
        flags = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        rows = np.full((n, 2 * S + 4), np.nan, np.float32) if want_rows else None
        run = [i for i in range(n) if (self.counters[i, 2] & 0xff) == RUNNING]
        for i in range(n):
            if i not in run:
                next_obs[i] = self.obs[i]
                status[i] = self.counters[i, 2]
        cmd = {}
        for i in run:
            cmd[i] = clip_command(actions[i], p)
            self.state[i, :3] = move(self.state[i], *cmd[i], p)
        respawned = []
        if run:
            scans = self._cast(self.state[run, :3])
        for k, i in enumerate(run):
            st, cn = self.state[i], self.counters[i]
            rx, ry, r, term, stat, thr = sarsa(st, scans[k], p)
            self.margin_thr = min(self.margin_thr, thr)
            cn[0] += 1
            trunc = cn[0] >= p["episode_step"]
            if not term and trunc:
                stat = TIMELIMITED
            o = obs_row(scans[k], st, rx, ry, self.layout)
            next_obs[i], reward[i], flags[i], status[i] = o, np.float32(r), int(term) | (int(trunc) << 1), stat
            if want_rows:
                rows[i] = np.concatenate([self.obs[i], [np.float32(r)], o, [np.float32(term)], np.array(cmd[i]).astype(np.float32)])
            if (term or trunc) and self.auto_reset:
                respawned.append((i, self._respawn(i)))
            else:
                cn[2] = stat
                self.obs[i] = o
        if respawned:
            idx = [i for i, _ in respawned]
            scans = self._cast(self.state[idx, :3])
            self.min_spawn_scan = min(self.min_spawn_scan, float(scans.min()))
            for k, (i, tail) in enumerate(respawned):
                self.obs[i] = obs_row(scans[k], self.state[i], *tail, self.layout)
        return dict(next_obs=next_obs, reward=reward, flags=flags, status=status, rows=rows)

    def margins(self):
        """Smallest distance of any decision met so far from its tie: (geometric, thresholds, reset rejections)."""
        return self.margin_geo, self.margin_thr, self.margin_reset


def margins(world, poses, p=PARAMS):
    """min over the geometric and range_max margins of a set of poses (scan cases)."""
    _, geo, thr = cast(world[0], world[1], poses, p, with_margin=True)
    return min(geo, thr)


# ---- cases --------------------------------------------------------------------------------------------------------------
def lattice_poses(n, seed, p=PARAMS):
    """n poses inside the lattice world at rank 0, away from pillars and walls, redrawn until every margin exceeds MARGIN."""
    world = lattice()
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x = p["origin_x"] + rng.integers(5) + rng.uniform(0.16, 0.84)
        y = p["origin_y"] + rng.integers(5) + rng.uniform(0.16, 0.84)
        pose = np.array([[x, y, rng.uniform(-math.pi, math.pi)]])
        if margins(world, pose, p) > MARGIN:
            out.append(pose[0])
    return np.array(out)


def oblique_poses(n, seed, p=PARAMS):
    world = oblique()
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        pose = np.array([[rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-math.pi, math.pi)]])
        d = np.hypot(world[1][:, 0] - pose[0, 0], world[1][:, 1] - pose[0, 1]) - world[1][:, 2]
        if d.min() > 0.02 and margins(world, pose, p) > MARGIN:          # outside every pillar
            out.append(pose[0])
    return np.array(out)


def steer_normalised(obs, n_beams=360):
    """The scripted agent as test.py's `select_action`: the action in [-1, 1]^2 whose command `(a + [1, 0]) * [0.075, 1.5]`
    is full speed and w = clip(2 atan2(gy, gx), +-1.5) on the goal in the robot frame ("goal" layout).  fp64."""
    gx, gy = obs[..., n_beams].astype(np.float64), obs[..., n_beams + 1].astype(np.float64)
    w = np.clip(2.0 * np.arctan2(gy, gx), -1.5, 1.5)
    return np.stack([np.ones_like(w), w / 1.5], axis=-1)


def steer(obs, n_beams=360):
    """The scripted agent's command `v, w` as the float32 the simulator is handed."""
    return ((steer_normalised(obs, n_beams) + np.array([1.0, 0.0])) * np.array([0.15 / 2, 1.5])).astype(np.float32)


ROLLOUT = dict(n=64, T=60, episode_step=40, seed=12345)


def rollout_commands(obs, t, n_beams=360):
    """Commands of the roll-out at step t: every third robot steers at the goal, the others drive uniform random commands
    (collect.py:38's rule) from a generator keyed by the step alone, so they do not depend on what the robots see."""
    a = steer(obs, n_beams)
    u = np.random.default_rng([ROLLOUT["seed"], t]).random((obs.shape[0], 2))
    rnd = ((u * 2 + np.array([0.0, -1.0])) * np.array([0.075, 1.5])).astype(np.float32)
    sel = np.arange(obs.shape[0]) % 3 != 0
    a[sel] = rnd[sel]
    return a


def rollout(auto_reset=True, layout="goal", **over):
    """The roll-out the GPU tests repeat step by step: returns (sim, per-step records, outcome counts)."""
    cfg = dict(ROLLOUT)
    cfg.update(over)
    p = params(episode_step=cfg["episode_step"])
    sim = Sim(lattice(), cfg["n"], seed=cfg["seed"], layout=layout, auto_reset=auto_reset, p=p)
    sim.reset()
    counts = {HIT: 0, GOAL: 0, TIMELIMITED: 0}
    steps = []
    for t in range(cfg["T"]):
        a = rollout_commands(sim.obs, t)
        before = (sim.state.copy(), sim.counters.copy(), sim.obs.copy())
        out = sim.step(a, want_rows=True)
        for k in counts:
            counts[k] += int((out["status"] == k).sum()) if auto_reset else 0
        steps.append(dict(actions=a, before=before, out=out, state=sim.state.copy(), counters=sim.counters.copy(),
                          obs=sim.obs.copy()))
    return sim, steps, counts
