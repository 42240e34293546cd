"""Writes tests/golden/expert_paths.npz: occupancy grids, start and goal cells, and the path the reference's planner returns.

    python tests/helpers/gen_expert_golden.py [reference_dir]

Runs on a CPU box with the reference checked out (default /root/reference); never on the GPU machine.  The planner is the
reference's UNMODIFIED dataloader/a_star.py `AStarPlanner`: constructed with empty `ox, oy` (which fixes its window to
[-10, 10] x [-5, 5] at the given resolution and leaves the map empty), its `obstacle_map` attribute then supplied from
outside, and `planning` called with the centres of the start and goal cells.  The scenes are
tests/helpers/expert_cases.py's `golden_scenes`.  Stored: the occupancy bits (np.packbits of `occ[ix, iy]`), start, goal and
`rx, ry` as returned (goal first), concatenated with offsets.  Only data.
"""
import contextlib
import io
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from helpers import expert_cases as EC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(HERE), "golden", "expert_paths.npz")


def _import_planner():
    for mod in ("matplotlib", "matplotlib.pyplot"):
        if mod not in sys.modules:
            try:
                __import__(mod)
            except Exception:
                m = types.ModuleType(mod)
                m.__path__ = []
                sys.modules[mod] = m
    sys.path.insert(0, os.path.join(REF, "dataloader"))
    import a_star
    return a_star.AStarPlanner


def main():
    Planner = _import_planner()
    g = EC.GOLDEN_GRID
    kinds, occs, starts, goals, rxs, rys, offsets = [], [], [], [], [], [], [0]
    for kind, occ, start, goal in EC.golden_scenes():
        planner = Planner([], [], g.res, 0.13)
        assert (planner.x_width, planner.y_width, planner.min_x, planner.min_y) == (g.w, g.h, g.min_x, g.min_y)
        planner.obstacle_map = occ.tolist()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            rx, ry = planner.planning(*g.centre(*start), *g.centre(*goal))
        dt = time.perf_counter() - t0
        kinds.append(kind)
        occs.append(np.packbits(occ.reshape(-1)))
        starts.append(start)
        goals.append(goal)
        rxs += list(rx)
        rys += list(ry)
        offsets.append(len(rxs))
        restated = len(EC.descend(EC.field(occ, goal), start, goal))
        print(f"{kind:18s} len(rx) = {len(rx):4d}  restated path_len = {restated:4d}  {dt:.2f} s", flush=True)
    np.savez_compressed(OUT, kind=np.array(kinds), occ=np.stack(occs), start=np.array(starts, np.int32),
                        goal=np.array(goals, np.int32), rx=np.array(rxs, np.float64), ry=np.array(rys, np.float64),
                        offsets=np.array(offsets, np.int64))
    print(f"{len(kinds)} scenes -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
