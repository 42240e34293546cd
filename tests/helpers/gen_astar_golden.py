"""Writes tests/golden/astar_rows.npz: transition rows and what the reference's labelling pass makes of them.

    python tests/helpers/gen_astar_golden.py [reference_dir]

Runs on a CPU box with the reference checked out (default /root/reference); never on the GPU machine.  Each row goes
through the reference's `preprocessing` (preprocess.py:11-68, planner dataloader/a_star.py:8-221) as float64, the way
`general_process` feeds it from np.loadtxt.  Recorded per row: whether it was kept, len(rx) of the planner's path, and
the value as the float32 the reference's tensor store makes of it.  Rows come from tests/helpers/astar_cases.py, which
redraws a row until no comparison in the pass sits within a margin of a tie; this script asserts that again.
"""
import contextlib
import io
import math
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import astar_cases as AC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(HERE), "golden", "astar_rows.npz")


def _import_reference():
    for mod in ("matplotlib", "matplotlib.pyplot"):
        if mod not in sys.modules:
            try:
                __import__(mod)
            except Exception:
                m = types.ModuleType(mod)
                m.__path__ = []
                sys.modules[mod] = m
    sys.path.insert(0, REF)
    import preprocess
    return preprocess


def cases():
    """(kind, seed, heading): the situations the fixture has to cover."""
    out = []
    for s in range(8):
        out.append(("pillar", s, None))
    for s in range(3):
        out.append(("behind_pillar", s, None))
    for kind in ("sealed_out", "sealed_in", "off_grid", "on_return", "start", "too_close", "open_far", "no_beam"):
        out += [(kind, 0, None), (kind, 1, None)]
    out += [("wall_gap", s, None) for s in range(4)]
    out += [("u_room", 0, None), ("u_room", 1, 0.3)]
    out += [("pillar", 100, math.pi - 0.01), ("pillar", 101, -math.pi + 0.01), ("u_room", 2, math.pi - 0.02),
            ("open_far", 2, -math.pi + 0.005)]
    return out


def main():
    pre = _import_reference()
    lens = []
    planning = pre.AStarPlanner.planning

    def recording(self, *a):
        rx, ry = planning(self, *a)
        lens.append(len(rx))
        return rx, ry

    pre.AStarPlanner.planning = recording
    rows, kept, path_len, value, kinds, secs = [], [], [], [], [], []
    for kind, seed, heading in cases():
        row = AC.make_row(kind, seed, heading)
        assert AC.margins_ok(row)
        lens.clear()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            got = pre.preprocessing(row.astype(np.float64))
        dt = time.perf_counter() - t0
        n = lens[0] if lens else 0
        rows.append(row)
        kept.append(got is not None)
        path_len.append(n)
        value.append(np.float32(got[360]) if got is not None else np.float32(0))
        kinds.append(kind)
        if lens:
            secs.append(dt)
        if got is not None:
            assert np.array_equal(got[:360], row[:360].astype(np.float64))
        print(f"{kind:14s} seed {seed:3d}: kept={got is not None} len={n} value={value[-1]!r} {dt:.2f}s "
              f"restated={AC.label(row)}", flush=True)
    path_len = np.array(path_len, dtype=np.int32)
    assert path_len[[k == "u_room" for k in kinds]].max() > 100, "no detour of more than 100 nodes"
    np.savez_compressed(OUT, rows=np.stack(rows).astype(np.float32), kept=np.array(kept), path_len=path_len,
                        value=np.array(value, dtype=np.float32), kind=np.array(kinds))
    print(f"{len(rows)} rows, {sum(kept)} kept -> {OUT}; reference planner: mean {np.mean(secs):.2f} s per row, "
          f"max {np.max(secs):.2f} s over {len(secs)} planned rows")


if __name__ == "__main__":
    main()
