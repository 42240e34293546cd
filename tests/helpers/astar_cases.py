"""The labelling pass (lidar scan -> occupancy grid -> 8-connected shortest path -> 15 * 0.99^len) restated in numpy,
and a deterministic generator of transition rows for it.

The restatement does not follow the planner's expansion order.  A cheapest 8-connected path costs a + b*sqrt(2) with `a`
axis moves and `b` diagonal moves; sqrt(2) is irrational, so every cheapest path has the same (a, b) and the same node
count a + b + 1, whatever the tie-breaking.  `label` therefore runs Dijkstra on exact integer pairs and compares them
through a + b*sqrt(2) evaluated afresh from the integers (two distinct pairs with a + b < 65536 differ by more than
1 / (65536 * 2.42) = 6e-6; the fp64 evaluation is good to 1e-11).

Status codes are the library's (include/porl_hip.h): 0 labelled, 1 a beam closer than the robot radius, 2 goal in the
start cell, 3 goal off the grid, 4 goal cell blocked, 5 goal unreachable, 6 non-finite goal.

`margins_ok` is what makes a row safe as a test vector: no range within 1e-6 of a threshold, no cell centre within
1e-6 of the inflation radius of a point, no goal coordinate within 1e-3 cells of a rounding boundary.  With these, two
correct fp64 implementations cannot disagree on a tie.  Generated rows are redrawn until the margins hold.
"""
import heapq
import math

import numpy as np

ROW_WIDTH = 734
SQRT2 = math.sqrt(2.0)

OK, TOO_CLOSE, GOAL_IS_START, GOAL_OFF_GRID, GOAL_BLOCKED, UNREACHABLE, NON_FINITE, NOT_CONVERGED = range(8)

DEFAULT = dict(resolution=0.1, robot_radius=0.13, min_x=-10.0, max_x=10.0, min_y=-5.0, max_y=5.0, range_lo=0.15,
               range_hi=3.5, n_beams=360, pose_offset=360, heading_offset=362, goal_offset=363)


def params(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


def grid_dims(p):
    return round((p["max_x"] - p["min_x"]) / p["resolution"]), round((p["max_y"] - p["min_y"]) / p["resolution"])


def start_cell(p):
    return round((0.0 - p["min_x"]) / p["resolution"]), round((0.0 - p["min_y"]) / p["resolution"])


def value_of(n):
    return np.float32(15.0 * np.power(0.99, n))


def goal_position(row, p):
    """Goal in the robot frame, in cell units before rounding (fp64 on the fp32 row's values)."""
    d = np.asarray(row, dtype=np.float64)
    po, ho, go = p["pose_offset"], p["heading_offset"], p["goal_offset"]
    h = d[ho]
    rel = d[go:go + 2] - d[po:po + 2]
    rot = np.array([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])
    g = np.matmul(rot, rel[:, None])[:, 0]
    return (g[0] - p["min_x"]) / p["resolution"], (g[1] - p["min_y"]) / p["resolution"]


def obstacle_points(row, p):
    d = np.asarray(row, dtype=np.float64)[:p["n_beams"]]
    deg = 360.0 / p["n_beams"]
    ang = np.array([(i * deg) * np.pi / 180 for i in range(p["n_beams"])])
    keep = (d < p["range_hi"]) & (d > p["range_lo"])
    return (np.cos(ang) * d)[keep], (np.sin(ang) * d)[keep]


def occupancy(ox, oy, p):
    """(W, H) bool map and the smallest | distance - radius | over every (cell centre, point) pair."""
    W, H = grid_dims(p)
    occ = np.zeros((W, H), dtype=bool)
    margin = np.inf
    X = np.arange(W) * p["resolution"] + p["min_x"]
    Y = np.arange(H) * p["resolution"] + p["min_y"]
    rr = p["robot_radius"]
    for x, y in zip(ox, oy):
        # only the cells near the point can be within the radius; the rest only bound the margin from far above
        i0, i1 = np.searchsorted(X, [x - rr - 1e-3, x + rr + 1e-3])
        j0, j1 = np.searchsorted(Y, [y - rr - 1e-3, y + rr + 1e-3])
        if i0 == i1 or j0 == j1:
            continue
        dist = np.hypot(x - X[i0:i1, None], y - Y[None, j0:j1])
        occ[i0:i1, j0:j1] |= dist <= rr
        margin = min(margin, float(np.abs(dist - rr).min()))
    return occ, margin


MOVES = ((1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (-1, -1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, 1))


def shortest_pair(occ, start, goal):
    """(a, b) of a cheapest path start -> goal over unblocked cells (the start itself is never checked), or None."""
    W, H = occ.shape
    free = (~occ).tolist()
    best = [[math.inf] * H for _ in range(W)]
    done = [[False] * H for _ in range(W)]
    best[start[0]][start[1]] = 0.0
    heap = [(0.0, 0, 0, start[0], start[1])]
    while heap:
        _, a, b, x, y = heapq.heappop(heap)
        if done[x][y]:
            continue
        done[x][y] = True
        if (x, y) == goal:
            return a, b
        for dx, dy, diag in MOVES:
            nx, ny = x + dx, y + dy
            if 0 <= nx < W and 0 <= ny < H and free[nx][ny] and not done[nx][ny]:
                na, nb = a + 1 - diag, b + diag
                c = na + nb * SQRT2
                if c < best[nx][ny] - 1e-7:
                    best[nx][ny] = c
                    heapq.heappush(heap, (c, na, nb, nx, ny))
    return None


def label(row, p=DEFAULT):
    """(status, path_len, value float32) of one row."""
    d = np.asarray(row, dtype=np.float64)
    zero = np.float32(0.0)
    if d[:p["n_beams"]].min() < p["robot_radius"]:          # numpy's min: a NaN beam makes the comparison false
        return TOO_CLOSE, 0, zero
    fx, fy = goal_position(row, p)
    if not (math.isfinite(fx) and math.isfinite(fy)):
        return NON_FINITE, 0, zero
    goal = (round(fx), round(fy))
    start = start_cell(p)
    W, H = grid_dims(p)
    if goal == start:
        return GOAL_IS_START, 0, zero
    if not (0 <= goal[0] < W and 0 <= goal[1] < H):
        return GOAL_OFF_GRID, 0, zero
    occ, _ = occupancy(*obstacle_points(row, p), p)
    if occ[goal]:
        return GOAL_BLOCKED, 0, zero
    ab = shortest_pair(occ, start, goal)
    if ab is None:
        return UNREACHABLE, 0, zero
    n = ab[0] + ab[1] + 1
    return OK, n, value_of(n)


def label_all(rows, p=DEFAULT):
    out = [label(r, p) for r in rows]
    return (np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.int32),
            np.array([o[2] for o in out], dtype=np.float32))


def margins_ok(row, p=DEFAULT):
    d = np.asarray(row, dtype=np.float64)
    scan = d[:p["n_beams"]]
    for t in (p["robot_radius"], p["range_lo"], p["range_hi"]):
        if np.abs(scan - t).min() <= 1e-6:
            return False
    fx, fy = goal_position(row, p)
    if math.isfinite(fx) and math.isfinite(fy):
        for f in (fx, fy):
            if abs((f - math.floor(f)) - 0.5) <= 1e-3:
                return False
    _, margin = occupancy(*obstacle_points(row, p), p)
    return margin > 1e-6


# ---- scenes -> scans ---------------------------------------------------------------------------------------------------
NO_RETURN = 4.0          # what a beam reads when nothing is within range


def cast(segments=(), circles=(), n_beams=360):
    """Ranges of n_beams rays from the origin against line segments (x1, y1, x2, y2) and circles (cx, cy, r)."""
    ang = np.arange(n_beams) * (2 * np.pi / n_beams)
    ux, uy = np.cos(ang), np.sin(ang)
    rng = np.full(n_beams, np.inf)
    for x1, y1, x2, y2 in segments:
        ex, ey = x2 - x1, y2 - y1
        den = ux * ey - uy * ex
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (x1 * ey - y1 * ex) / den                 # along the ray
            s = (x1 * uy - y1 * ux) / den                 # along the segment
        hit = (np.abs(den) > 1e-12) & (t > 0) & (s >= 0) & (s <= 1)
        rng = np.where(hit & (t < rng), t, rng)
    for cx, cy, r in circles:
        bq = ux * cx + uy * cy
        disc = bq * bq - (cx * cx + cy * cy - r * r)
        with np.errstate(invalid="ignore"):
            t = bq - np.sqrt(disc)
        hit = (disc >= 0) & (t > 0)
        rng = np.where(hit & (t < rng), t, rng)
    return np.where(np.isfinite(rng), rng, NO_RETURN)


def box(x0, y0, x1, y1):
    return [(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]


def assemble(scan, goal_xy, heading, pose, rng, width=ROW_WIDTH, p=DEFAULT):
    """A transition row whose robot-frame goal is goal_xy: goal_world = pose + R(heading)^T goal_xy."""
    row = rng.uniform(-1, 1, width).astype(np.float32)          # the columns the pass never reads hold anything
    row[:p["n_beams"]] = scan
    c, s = math.cos(heading), math.sin(heading)
    gx, gy = goal_xy
    po, ho, go = p["pose_offset"], p["heading_offset"], p["goal_offset"]
    row[po:po + 2] = pose
    row[ho] = heading
    row[go] = pose[0] + c * gx - s * gy
    row[go + 1] = pose[1] + s * gx + c * gy
    return row


KINDS = ("pillar", "behind_pillar", "sealed_out", "sealed_in", "off_grid", "on_return", "start", "too_close", "open_far",
         "u_room", "no_beam", "wall_gap")


def scene(kind, rng):
    """(scan, robot-frame goal) of one situation; every draw differs, so a redraw moves every margin."""
    jit = lambda a=0.02: float(rng.uniform(-a, a))
    if kind == "pillar":
        scan = cast(box(-2.4 + jit(), -2.1 + jit(), 2.6 + jit(), 2.2 + jit()), [(1.0 + jit(), 0.1 + jit(), 0.3)])
        goal = (rng.uniform(-2.0, 2.0), rng.uniform(-1.7, 1.7))
    elif kind == "behind_pillar":
        scan = cast(box(-2.4 + jit(), -2.1 + jit(), 2.6 + jit(), 2.2 + jit()), [(1.0 + jit(), 0.0 + jit(), 0.35)])
        goal = (2.0 + jit(0.2), jit(0.2))
    elif kind == "sealed_out":
        scan = cast(box(-1.0 + jit(), -1.0 + jit(), 1.0 + jit(), 1.0 + jit()))
        goal = (rng.uniform(2.0, 6.0) * rng.choice([-1, 1]), rng.uniform(-3.0, 3.0))
    elif kind == "sealed_in":
        scan = cast(box(-1.0 + jit(), -1.0 + jit(), 1.0 + jit(), 1.0 + jit()))
        goal = (rng.uniform(-0.6, 0.6), rng.uniform(0.25, 0.6) * rng.choice([-1, 1]))
    elif kind == "off_grid":
        scan = cast(box(-2.4 + jit(), -2.1 + jit(), 2.6 + jit(), 2.2 + jit()))
        goal = (rng.uniform(-3.0, 3.0), rng.uniform(5.3, 7.0) * rng.choice([-1, 1]))
    elif kind == "on_return":
        scan = cast(box(-2.4 + jit(), -2.1 + jit(), 2.6 + jit(), 2.2 + jit()))
        i = int(rng.integers(0, 360))
        goal = (math.cos(math.radians(i)) * scan[i], math.sin(math.radians(i)) * scan[i])
    elif kind == "start":
        scan = cast(box(-2.4 + jit(), -2.1 + jit(), 2.6 + jit(), 2.2 + jit()))
        goal = (jit(0.03), jit(0.03))
    elif kind == "too_close":
        scan = cast(box(-2.4 + jit(), -2.1 + jit(), 2.6 + jit(), 2.2 + jit()))
        scan[int(rng.integers(0, 360))] = 0.12 + jit(0.005)
        goal = (1.0 + jit(), 1.0 + jit())
    elif kind == "open_far":
        scan = np.full(360, NO_RETURN)
        goal = (rng.uniform(5.0, 7.5) * rng.choice([-1, 1]), rng.uniform(-4.0, 4.0))
    elif kind == "no_beam":                                   # nothing in (range_lo, range_hi): an empty map
        scan = np.where(rng.random(360) < 0.5, 0.14 + rng.uniform(0.0, 0.005, 360), NO_RETURN + rng.uniform(0, 1, 360))
        goal = (rng.uniform(-6.0, 6.0), rng.uniform(-3.0, 3.0))
    elif kind == "u_room":                                    # open only behind the robot, goal straight ahead
        f, s, back = 1.2 + jit(), 1.3 + jit(), -3.15 + jit()
        scan = cast([(f, -s, f, s), (f, s, back, s), (f, -s, back, -s)])
        goal = (3.6 + jit(0.3), jit(0.3))
    elif kind == "wall_gap":                                  # a wall ahead with one gap far to the side
        x, g = 1.0 + jit(), rng.uniform(1.6, 2.2) * rng.choice([-1, 1])
        lo, hi = sorted((g - 0.35 * np.sign(g), g + 0.35 * np.sign(g)))
        scan = cast([(x, -3.2, x, lo), (x, hi, x, 3.2), (x, 3.2, -0.5, 3.2), (x, -3.2, -0.5, -3.2)])
        goal = (2.5 + jit(0.3), -0.5 * np.sign(g) + jit(0.3))
    else:
        raise ValueError(kind)
    scan = np.asarray(scan, dtype=np.float64)
    real = scan < NO_RETURN
    scan = np.where(real & (kind != "no_beam"), scan + rng.normal(0, 0.003, scan.shape), scan)   # sensor noise
    return scan, goal


def make_row(kind, seed, heading=None, p=DEFAULT, width=ROW_WIDTH):
    """Deterministic in (kind, seed); redrawn until the margins hold — never skipped."""
    for attempt in range(1000):
        rng = np.random.default_rng([seed, attempt, KINDS.index(kind)])
        scan, goal = scene(kind, rng)
        h = float(rng.uniform(-math.pi, math.pi)) if heading is None else heading
        row = assemble(scan, goal, h, rng.uniform(-5, 5, 2), rng, width, p)
        if margins_ok(row, p):
            return row
    raise RuntimeError(f"no draw of {kind}/{seed} met the margins")


def make_rows(n, seed=0, p=DEFAULT, width=ROW_WIDTH):
    return np.stack([make_row(KINDS[i % len(KINDS)], seed * 100003 + i, p=p, width=width) for i in range(n)])


def empty_field_row(dx, dy, p=DEFAULT, width=ROW_WIDTH):
    """Nothing in range, heading 0, robot at the origin, goal in the centre of the cell (dx, dy) away from the start."""
    row = np.zeros(width, dtype=np.float32)
    row[:p["n_beams"]] = NO_RETURN
    go = p["goal_offset"]
    row[go], row[go + 1] = dx * p["resolution"], dy * p["resolution"]
    return row
