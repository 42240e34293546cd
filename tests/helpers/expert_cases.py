"""The A* expert of csrc/expert.hpp in fp64 numpy, in this project's own words: rasterise, field, descent, steer, scores,
the case generators, and the distance of every discontinuous decision from its tie.  Tests compare the device per cell
and per element against this file on cases whose margins exceed MARGIN, so two correct implementations cannot disagree
on a decision.

Arithmetic is written operation for operation as the kernels' (which compile without fused multiply-adds): products,
sums and quotients agree bit for bit; hypot / atan2 / cos may differ by an ulp of fp64.  Fields are exact integer pairs
(a << 16 | b), so they and every descent agree exactly.
"""
import math

import numpy as np

MARGIN = 1e-9
GAP = 1e-6                       # rows whose top two scores are closer than this are left out of the arg-max comparison
SQRT2 = 1.4142135623730951
UNREACHED = 0xFFFFFFFF
MOVES = ((1, 0), (0, 1), (-1, 0), (0, -1), (-1, -1), (-1, 1), (1, -1), (1, 1))     # the reference's motion order
OK, NO_FIELD, GOAL_OFF_GRID, GOAL_BLOCKED, NON_FINITE, NOT_CONVERGED = range(6)
PARAMS = dict(dt=0.2, max_lin_vel=0.15, max_ang_vel=1.5, n_actions=5, ang_step=0.75)


class Grid:
    def __init__(self, res, inflate, min_x, min_y, w, h):
        self.res, self.inflate, self.min_x, self.min_y, self.w, self.h = float(res), float(inflate), float(min_x), float(min_y), w, h
        self.pw, self.pcells = w + 2, (w + 2) * (h + 2)

    def kwargs(self):
        return dict(resolution=self.res, inflate=self.inflate, min_x=self.min_x, min_y=self.min_y, w=self.w, h=self.h)

    def centre(self, ix, iy):
        return ix * self.res + self.min_x, iy * self.res + self.min_y


def lattice_grid(origin=(-10.0, 5.0), res=0.1, inflate=0.18, cells=5):
    side = round(cells / res) + 1
    return Grid(res, inflate, origin[0], origin[1], side, side)


def cost(v):
    return (v >> 16) + (v & 0xFFFF) * SQRT2


# ---- rasterise ----------------------------------------------------------------------------------------------------------
def rasterize(segments, circles, g):
    """(occ (w, h) bool `[ix, iy]`, margin): blocked iff the cell centre lies within `inflate` of a primitive; margin = the
    smallest |d - inflate| over all cell and primitive pairs."""
    seg = np.asarray(segments, np.float32).reshape(-1, 4).astype(np.float64)
    cir = np.asarray(circles, np.float32).reshape(-1, 3).astype(np.float64)
    cx = (np.arange(g.w, dtype=np.float64) * g.res + g.min_x)[:, None, None]
    cy = (np.arange(g.h, dtype=np.float64) * g.res + g.min_y)[None, :, None]
    occ = np.zeros((g.w, g.h), bool)
    margin = math.inf
    if len(seg):
        ax, ay = seg[:, 0], seg[:, 1]
        ex, ey = seg[:, 2] - ax, seg[:, 3] - ay
        ee = ex * ex + ey * ey
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((cx - ax) * ex + (cy - ay) * ey) / ee
        t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
        point = np.broadcast_to(ee == 0.0, t.shape)
        qx = np.where(point, ax, ax + t * ex)
        qy = np.where(point, ay, ay + t * ey)
        d = np.hypot(cx - qx, cy - qy)
        occ |= (d <= g.inflate).any(axis=2)
        margin = min(margin, float(np.abs(d - g.inflate).min()))
    if len(cir):
        d = np.hypot(cx - cir[:, 0], cy - cir[:, 1]) - cir[:, 2]
        occ |= (d <= g.inflate).any(axis=2)
        margin = min(margin, float(np.abs(d - g.inflate).min()))
    return occ, margin


def pack_bitmap(occ):
    """The device's bitmap of an occupancy array: bit (iy + 1) * (w + 2) + ix + 1 of uint32 words, halo 0."""
    w, h = occ.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = occ.T
    bits = pad.reshape(-1)
    words = np.zeros((bits.size + 31) // 32 * 32, np.uint64)
    words[:bits.size] = bits
    words = (words.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1)
    return words.astype(np.uint32)


def unpack_interior(words, g):
    """(w, h) bool from the device's bitmap: the interior bits only (halo bits may hold anything)."""
    words = np.asarray(words).astype(np.uint32)
    p = np.arange(g.pcells)
    bits = (words[p >> 5] >> (p & 31).astype(np.uint32)) & 1
    return bits.reshape(g.h + 2, g.pw)[1:-1, 1:-1].T.astype(bool)


# ---- cells, field, descent --------------------------------------------------------------------------------------------------
def cell_of(g, x, y):
    """(code, ix, iy, margin): OK with the cell, NON_FINITE, or GOAL_OFF_GRID for "off the grid"; margin = the distance of
    either quotient from a half."""
    with np.errstate(all="ignore"):
        qx, qy = (np.float64(x) - g.min_x) / g.res, (np.float64(y) - g.min_y) / g.res
        fx, fy = np.rint(qx), np.rint(qy)
    if not (np.isfinite(fx) and np.isfinite(fy)):
        return NON_FINITE, 0, 0, math.inf
    margin = min(abs(qx - math.floor(qx) - 0.5), abs(qy - math.floor(qy) - 0.5))
    if fx < 0 or fx >= g.w or fy < 0 or fy >= g.h:
        return GOAL_OFF_GRID, 0, 0, margin
    return OK, int(fx), int(fy), margin


def field(occ, goal):
    """(w, h) uint32 `[ix, iy]`: the exact pair a << 16 | b of a cheapest 8-connected path to `goal` through free cells,
    UNREACHED elsewhere.  Relaxation to the fixpoint on exact integer pairs (all cheapest paths share their pair: sqrt 2
    is irrational)."""
    w, h = occ.shape
    free = np.zeros((w + 2, h + 2), bool)
    free[1:-1, 1:-1] = ~occ
    free[goal[0] + 1, goal[1] + 1] = False                      # holds (0, 0) for good
    A = np.zeros((w + 2, h + 2), np.int64)
    B = np.zeros((w + 2, h + 2), np.int64)
    c = np.full((w + 2, h + 2), np.inf)
    c[goal[0] + 1, goal[1] + 1] = 0.0
    for _ in range(w * h + 1):
        bc, bA, bB = c.copy(), A.copy(), B.copy()
        for k, (dx, dy) in enumerate(MOVES):
            nA = np.roll(A, (-dx, -dy), axis=(0, 1)) + (1 if k < 4 else 0)
            nB = np.roll(B, (-dx, -dy), axis=(0, 1)) + (0 if k < 4 else 1)
            reached = np.isfinite(np.roll(c, (-dx, -dy), axis=(0, 1)))
            nc = np.where(reached, nA + nB * SQRT2, np.inf)
            better = free & (nc < bc)
            bc, bA, bB = np.where(better, nc, bc), np.where(better, nA, bA), np.where(better, nB, bB)
        if np.array_equal(bc, c):
            break
        c, A, B = bc, bA, bB
    else:
        raise AssertionError("no fixpoint")
    out = np.where(np.isfinite(c), (A << 16) | B, UNREACHED).astype(np.uint32)
    return out[1:-1, 1:-1]


def pairs(fld):
    """(a, b) int32 arrays of a field, -1 where unreached: what AStarExpert.field returns."""
    un = fld == UNREACHED
    return np.where(un, -1, fld >> 16).astype(np.int32), np.where(un, -1, fld & 0xFFFF).astype(np.int32)


def _at(fld, ix, iy):
    w, h = fld.shape
    return int(fld[ix, iy]) if 0 <= ix < w and 0 <= iy < h else UNREACHED


def descend(fld, start, goal):
    """The cells from `start` (reached or not) to `goal`, both included, by the motion-order rule; [] when there is none."""
    cur = tuple(start)
    path = [cur]
    v = _at(fld, *cur)
    if v == UNREACHED:
        best = None
        for dx, dy in MOVES:
            n = (cur[0] + dx, cur[1] + dy)
            vn = _at(fld, *n)
            if vn != UNREACHED and (best is None or cost(vn) < cost(best[1])):
                best = (n, vn)
        if best is None:
            return []
        cur, v = best
        path.append(cur)
    while cur != tuple(goal):
        for k, (dx, dy) in enumerate(MOVES):
            n = (cur[0] + dx, cur[1] + dy)
            vn = _at(fld, *n)
            if vn != UNREACHED and vn + (0x10000 if k < 4 else 1) == v:
                cur, v = n, vn
                path.append(cur)
                break
        else:
            raise AssertionError(f"no descent from {cur}: not a fixpoint")
    return path


class Planner:
    """The expert on one grid: fields are cached per goal cell, as the device caches them per robot."""

    def __init__(self, g, occ, lookahead=2, p=PARAMS):
        self.g, self.occ, self.lookahead, self.p = g, occ, lookahead, p
        self._fields = {}
        self.margin = math.inf

    def field_of(self, cell):
        if cell not in self._fields:
            self._fields[cell] = field(self.occ, cell)
        return self._fields[cell]

    def goal_cell(self, st):
        """(status, cell): OK with the goal cell when the device would hold a field for this state's goal."""
        code, ix, iy, m = cell_of(self.g, st[3], st[4])
        if code != OK:
            return (NON_FINITE if code == NON_FINITE else GOAL_OFF_GRID), None
        self.margin = min(self.margin, m)
        if self.occ[ix, iy]:
            return GOAL_BLOCKED, None
        return OK, (ix, iy)

    def plan(self, st, max_path=0):
        """dict(status, waypoint, path_len, path (max_path, 2) int32) of one robot's state `x y yaw gx gy ...`."""
        g = self.g
        out = dict(status=OK, waypoint=(float(st[3]), float(st[4])), path_len=0, path=np.full((max_path, 2), -1, np.int32))
        if not all(math.isfinite(v) for v in st[:3]):
            out["status"] = NON_FINITE
            return out
        status, goal = self.goal_cell(st)
        if status != OK:
            out["status"] = status
            return out
        code, rix, riy, m = cell_of(g, st[0], st[1])
        if code != OK:
            out["status"] = NON_FINITE if code == NON_FINITE else NO_FIELD
            return out
        self.margin = min(self.margin, m)
        cells = descend(self.field_of(goal), (rix, riy), goal)
        if not cells:
            out["status"] = NO_FIELD
            return out
        out["path_len"] = len(cells)
        k = min(self.lookahead, len(cells) - 1)
        if cells[k] != goal:
            out["waypoint"] = g.centre(*cells[k])
        n = min(max_path, len(cells))
        if n:
            out["path"][:n] = cells[:n]
        return out

    # ---- steer ----
    def error(self, st, wp):
        """The heading error to the waypoint, wrapped as navd_tail wraps; its margin is the raw difference's distance from
        +-pi."""
        raw = math.atan2(wp[1] - st[1], wp[0] - st[0]) - st[2]
        self.margin = min(self.margin, abs(raw - math.pi), abs(raw + math.pi))
        if raw > math.pi:
            raw -= 2.0 * math.pi
        elif raw < -math.pi:
            raw += 2.0 * math.pi
        return raw

    def command(self, st, plan):
        if plan["status"] == NON_FINITE:
            return 0.0, 0.0
        p = self.p
        e = self.error(st, plan["waypoint"])
        om = e / p["dt"]
        om = -p["max_ang_vel"] if om < -p["max_ang_vel"] else (p["max_ang_vel"] if om > p["max_ang_vel"] else om)
        c = math.cos(e)
        return p["max_lin_vel"] * (c if c > 0.0 else 0.0), om

    def scores(self, st, plan):
        p = self.p
        A = p["n_actions"]
        if plan["status"] == NON_FINITE:
            return np.zeros(A)
        e = self.error(st, plan["waypoint"])
        return np.array([-abs(e - ((A - 1) / 2.0 - a) * p["ang_step"] * p["dt"]) for a in range(A)])

    def act(self, states, max_path=0):
        """Everything the device returns for (n, 8) states: dict of arrays (commands and scores in fp64)."""
        plans = [self.plan(st, max_path) for st in states]
        return dict(status=np.array([q["status"] for q in plans], np.int32),
                    path_len=np.array([q["path_len"] for q in plans], np.int32),
                    waypoint=np.array([q["waypoint"] for q in plans], np.float64),
                    path=np.stack([q["path"] for q in plans]) if len(plans) else np.zeros((0, max_path, 2), np.int32),
                    commands=np.array([self.command(st, q) for st, q in zip(states, plans)], np.float64),
                    scores=np.stack([self.scores(st, q) for st, q in zip(states, plans)]))


def gap_rows(scores):
    """Rows whose top two scores are at least GAP apart: the arg-max is compared on these."""
    s = np.sort(np.asarray(scores, np.float64), axis=1)
    return (s[:, -1] - s[:, -2]) >= GAP


# ---- worlds and cases ---------------------------------------------------------------------------------------------------------
def lattice_world():
    from helpers import navsim_cases as NC
    return NC.lattice()


def room_world(origin=(-10.0, 5.0)):
    """The lattice world with a sealed room: a box of four walls [2.2, 2.8]^2 inside one lattice cell; at inflate 0.18 its
    free interior is the 3 x 3 cells 2.4 .. 2.6."""
    seg, cir = lattice_world()
    ox, oy = origin
    a, b = 2.2, 2.8
    box = [[ox + a, oy + a, ox + b, oy + a], [ox + b, oy + a, ox + b, oy + b], [ox + b, oy + b, ox + a, oy + b],
           [ox + a, oy + b, ox + a, oy + a]]
    return np.concatenate([seg, np.array(box, np.float32)]), cir


def tiny_world():
    """A 5 x 7 grid's world: a slanted wall, a degenerate segment (a point) and a pillar."""
    seg = np.array([[0.3, 2.6, 1.4, 3.1], [1.9, 0.45, 1.9, 0.45]], np.float32)
    cir = np.array([[0.4, 1.1, 0.2]], np.float32)
    return seg, cir


def tiny_grid():
    return Grid(0.5, 0.3, 0.0, 0.0, 5, 7)


def oblique_grid():
    return Grid(0.1, 0.18, -3.5, -3.3, 70, 66)               # 72 * 68 = 4896 padded cells: 153 whole words


def oblique_odd_grid():
    return Grid(0.1, 0.18, -3.45, -3.25, 69, 65)             # 71 * 67 = 4757 padded cells: no multiple of 32 or 64


def state_rows(rows):
    """(n, 8) fp64 states from (x, y, yaw, gx, gy) tuples."""
    st = np.zeros((len(rows), 8))
    st[:, :5] = np.array(rows, np.float64)
    return st


def field_states(origin=(-10.0, 5.0)):
    """Eight robots in `room_world`, one per situation: 0 an open goal; 1 a goal next to the wall; 2 a goal in the sealed
    room, robot outside (NO_FIELD); 3 robot and goal both in the room; 4 a goal on a pillar (blocked); 5 a goal off the
    grid; 6 a non-finite goal; 7 a robot on a blocked cell beside a pillar (the neighbour rule)."""
    ox, oy = origin
    nan = float("nan")
    return state_rows([
        (ox + 0.53, oy + 0.61, 0.3, ox + 3.47, oy + 4.22, ),
        (ox + 4.41, oy + 1.38, -2.0, ox + 0.22, oy + 3.51),
        (ox + 1.52, oy + 3.33, 1.0, ox + 2.52, oy + 2.41),
        (ox + 2.43, oy + 2.58, 2.5, ox + 2.61, oy + 2.39),
        (ox + 0.66, oy + 0.47, 0.0, ox + 3.02, oy + 1.97),
        (ox + 0.66, oy + 1.47, 0.0, ox + 5.31, oy + 1.2),
        (ox + 3.5, oy + 0.5, 0.0, nan, oy + 1.0),
        (ox + 1.12, oy + 1.22, -1.0, ox + 4.48, oy + 4.53),
    ])


def status_states(origin=(-10.0, 5.0)):
    """`field_states` and four more: 8 a non-finite pose, 9 a non-finite yaw, 10 a robot off the grid, 11 a robot whose cell
    is the goal's."""
    ox, oy = origin
    more = state_rows([
        (float("inf"), oy + 0.5, 0.0, ox + 1.5, oy + 1.5),
        (ox + 0.5, oy + 0.5, float("nan"), ox + 1.5, oy + 1.5),
        (ox - 0.4, oy + 0.5, 0.7, ox + 1.5, oy + 1.5),
        (ox + 1.52, oy + 1.49, 0.7, ox + 1.48, oy + 1.53),
    ])
    return np.concatenate([field_states(origin), more])


STATUS_WANT = [OK, OK, NO_FIELD, OK, GOAL_BLOCKED, GOAL_OFF_GRID, NON_FINITE, OK, NON_FINITE, NON_FINITE, NO_FIELD, OK]


def random_states(n, seed, g, occ, planner=None, p=PARAMS):
    """n robots with free start and goal cells drawn in the grid's window, each redrawn until every decision of its plan and
    command keeps MARGIN from its tie and its commands and scores keep GAP from 0 (so an fp64 ulp in atan2 or cos cannot move
    the fp32 result by more than its last place).  Score ties are not redrawn: `gap_rows` leaves them out of the arg-max
    comparison."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        xy = rng.uniform([g.min_x, g.min_y], [g.min_x + (g.w - 1) * g.res, g.min_y + (g.h - 1) * g.res], (2, 2))
        st = state_rows([(xy[0, 0], xy[0, 1], rng.uniform(-math.pi, math.pi), xy[1, 0], xy[1, 1])])[0]
        pl = Planner(g, occ, planner.lookahead if planner else 2, p)
        if planner:
            pl._fields = planner._fields
        cs, ix, iy, _ = cell_of(g, st[0], st[1])
        cg, jx, jy, _ = cell_of(g, st[3], st[4])
        if cs != OK or cg != OK or occ[ix, iy] or occ[jx, jy]:
            continue
        q = pl.plan(st)
        v, om = pl.command(st, q)
        s = pl.scores(st, q)
        if pl.margin > MARGIN and min(abs(om), abs(math.cos(pl.error(st, q["waypoint"])))) > GAP and np.abs(s).min() > GAP:
            out.append(st)
    return np.array(out)


# ---- the scenes of tests/golden/expert_paths.npz (tests/helpers/gen_expert_golden.py) ------------------------------------------
GOLDEN_GRID = Grid(0.1, 0.0, -10.0, -5.0, 200, 100)          # the window of the reference's calc_obstacle_map


def golden_scenes():
    """[(kind, occ (200, 100) bool, start cell, goal cell)]: start and goal free in every scene."""
    W, H = GOLDEN_GRID.w, GOLDEN_GRID.h
    out = []
    empty = np.zeros((W, H), bool)
    out.append(("open", empty.copy(), (20, 20), (150, 70)))
    out.append(("open_far", empty.copy(), (0, 0), (199, 99)))
    out.append(("diagonal", empty.copy(), (10, 10), (80, 80)))
    out.append(("adjacent_axis", empty.copy(), (50, 50), (50, 51)))
    out.append(("adjacent_diagonal", empty.copy(), (50, 50), (51, 49)))
    out.append(("same_cell", empty.copy(), (33, 44), (33, 44)))
    occ = empty.copy()
    occ[60:63, :] = True
    occ[60:63, 70:74] = False
    occ[120:123, :] = True
    occ[120:123, 12:15] = False
    occ[120:123, 90:92] = False
    out.append(("walls_with_gaps", occ, (10, 50), (190, 50)))
    occ = empty.copy()
    occ[100:102, 0:90] = True
    out.append(("detour", occ, (90, 10), (110, 10)))
    occ = empty.copy()
    occ[95:116, 20] = True
    occ[95, 20:41] = True
    occ[115, 20:41] = True
    out.append(("u_room", occ, (105, 10), (105, 30)))
    rng = np.random.default_rng(11)
    occ = empty.copy()
    for _ in range(60):
        x, y = rng.integers(5, W - 10), rng.integers(5, H - 10)
        occ[x:x + rng.integers(1, 7), y:y + rng.integers(1, 7)] = True
    occ[8:11, 8:11] = False
    occ[185:188, 88:91] = False
    out.append(("blocks", occ, (9, 9), (186, 89)))
    occ = empty.copy()
    occ[40:51, 40] = occ[40:51, 50] = True
    occ[40, 40:51] = occ[50, 40:51] = True
    out.append(("sealed_start", occ, (45, 45), (120, 60)))
    for kind, occ, s, g in out:
        assert not occ[s] and not occ[g], kind
    return out
