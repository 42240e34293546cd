"""A* path-value labels on the device — the pass the reference runs between the CSV shards and the value dataset
(/root/reference/preprocess.py:11-68 `preprocessing` on dataloader/a_star.py:8-221 `AStarPlanner`; the same pass in
`CustomDataset.__init__`, dataloader/dataloader.py:18-30).

Per transition row `[scan (n_beams) | ... pose, heading, goal ...]`: the scan becomes obstacle points, the points an
occupancy grid (cells within `robot_radius` of a point are blocked), and the row is labelled
`15 * 0.99 ** len(path)` for a cheapest 8-connected path from the robot's cell to the goal's.  Rows with a beam closer
than `robot_radius`, or without a path, are dropped.  One workgroup per row does all of it in LDS
(csrc/astar.hpp); the reference's pure-Python pass takes seconds per row.

    astar_values(rows)        -> (value, path_len, status) per row
    label_rows(rows)          -> (M, n_beams + 1) `[scan | value]` of the rows the reference keeps, in input order
    label_dataset(dataset)    -> DeviceDataset of those records, ready for EpochLoader

`status` (STATUS_NAMES): 0 labelled, 1 a beam closer than robot_radius, 2 goal in the robot's cell, 3 goal off the grid,
4 goal cell blocked, 5 goal unreachable, 6 non-finite goal, 7 not converged.  The reference drops 1-5 (returns None).
Where it raises — `round()` of a NaN or infinite goal coordinate — the row gets status 6 instead and is dropped too.
Status 7 means the kernel's sweep bound was hit; no input should produce it, and `label_rows` raises if one does.

Bit-exactness with the reference's float32 store: beam directions and the value table are built on the host exactly
as the reference forms them (`np.cos(i * np.pi / 180)`, `15. * np.power(0.99, n)` -> float32) and handed to the kernel,
which does its geometry in fp64 on the fp32 row's values and takes no `cos` of a constant and no `pow` itself.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native as N
from .dataloader import DeviceDataset

DEFAULTS = dict(resolution=0.1, robot_radius=0.13, min_x=-10.0, max_x=10.0, min_y=-5.0, max_y=5.0, range_lo=0.15,
                range_hi=3.5, n_beams=360, pose_offset=360, heading_offset=362, goal_offset=363)
STATUS_NAMES = ("labelled", "too_close", "goal_is_start", "goal_off_grid", "goal_blocked", "unreachable", "non_finite",
                "not_converged")
GOAL_REWARD, DECAY = 15.0, 0.99          # preprocess.py:58-59

_tables: dict = {}


def _params(kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown parameter(s) {sorted(unknown)}; known: {sorted(DEFAULTS)}")
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def grid_cells(**params):
    """Cells per axis (x, y) of a parameter set, counted as the reference counts them."""
    p = _params(params)
    return round((p["max_x"] - p["min_x"]) / p["resolution"]), round((p["max_y"] - p["min_y"]) / p["resolution"])


def _device_tables(p, device):
    """(beam directions (n_beams, 2) fp64, value table fp32) on `device`.  Scalar numpy calls on purpose: these are the
    calls the reference makes, and numpy's array loops may round differently from its scalar paths."""
    n_beams = int(p["n_beams"])
    w, h = grid_cells(**p)
    n_values = max(w * h, 0) + 2
    key = (str(device), n_beams, n_values)
    if key not in _tables:
        deg = 360.0 / n_beams                                                    # 1.0 for the reference's scan
        dirs = np.array([[np.cos((i * deg) * np.pi / 180), np.sin((i * deg) * np.pi / 180)] for i in range(n_beams)],
                        dtype=np.float64)
        vals = np.array([np.float32(GOAL_REWARD * np.power(DECAY, n)) for n in range(n_values)], dtype=np.float32)
        _tables[key] = (torch.from_numpy(dirs).to(device), torch.from_numpy(vals).to(device))
    return _tables[key]


def astar_values(rows, return_sweeps=False, **params):
    """Label every row of a (N, width) fp32 device tensor.  Returns (value fp32, path_len int32, status int32), each
    (N,); with `return_sweeps` also the relaxation sweeps each row took.  Rows may be a strided view (any row stride,
    unit column stride): nothing is copied.  Keyword parameters: see DEFAULTS (the reference's values)."""
    p = _params(params)
    if rows.device.type != "cuda":
        raise N.NativeError("astar_values runs on a HIP device only (no CPU path)")
    if rows.dim() != 2 or rows.dtype != torch.float32:
        raise ValueError(f"rows: expected (N, width) float32, got {rows.dtype} {tuple(rows.shape)}")
    if rows.shape[0] > 0 and rows.shape[1] > 1 and rows.stride(1) != 1:
        raise ValueError("rows must have unit column stride (slice rows or leading columns of a packed buffer)")
    need = max(p["n_beams"], p["pose_offset"] + 2, p["heading_offset"] + 1, p["goal_offset"] + 2)
    if rows.shape[1] < need:
        raise ValueError(f"rows are {rows.shape[1]} wide; the pass reads up to column {need}")
    n, dev = rows.shape[0], rows.device
    value = torch.empty(n, dtype=torch.float32, device=dev)
    path_len = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    sweeps = torch.empty(n, dtype=torch.int32, device=dev) if return_sweeps else None
    if n > 0:
        cp = N.AstarParams(p["resolution"], p["robot_radius"], p["min_x"], p["max_x"], p["min_y"], p["max_y"],
                           p["range_lo"], p["range_hi"], p["n_beams"], p["pose_offset"], p["heading_offset"],
                           p["goal_offset"])
        lib = N.lib()
        # a grid the library will refuse needs no tables: let the call name the argument
        try:
            w, h = grid_cells(**p)
        except (ArithmeticError, ValueError):
            w = h = 0
        if 0 < w * h <= 1 << 16:
            dirs, table = _device_tables(p, dev)
        else:
            dirs = table = torch.empty(1, dtype=torch.float64, device=dev)
        # the row stride of a one-row view is arbitrary; the kernel never steps past row 0 then
        stride = rows.stride(0) if n > 1 else max(rows.stride(0), rows.shape[1])
        N.check(lib.porl_astar_label(N.ptr(rows), stride, n, cp, N.ptr(dirs), N.ptr(table), table.numel(), N.ptr(value),
                                     N.ptr(path_len), N.ptr(status), N.ptr(sweeps), N.current_stream_ptr(rows)),
                "porl_astar_label")
    return (value, path_len, status, sweeps) if return_sweeps else (value, path_len, status)


def label_rows(rows, **params):
    """The reference's record `[scan | value]`, (M, n_beams + 1) fp32, for the rows it keeps (status 0), in input
    order."""
    p = _params(params)
    value, _, status = astar_values(rows, **p)
    if bool((status == 7).any()):
        raise N.NativeError("astar: a row hit the sweep bound (status 7, not converged); this is a bug, please report "
                            "the row")
    keep = status == 0
    return torch.cat([rows[:, :p["n_beams"]][keep], value[keep].unsqueeze(1)], dim=1)


def label_dataset(dataset, chunk_rows=1 << 16, **params):
    """Label a DeviceDataset of transition rows chunk by chunk (the per-row outputs never exceed `chunk_rows`) and return
    the value dataset — a DeviceDataset of width n_beams + 1 holding the kept rows in storage order."""
    if chunk_rows < 1:
        raise ValueError("chunk_rows must be positive")
    p = _params(params)
    src = dataset.rows
    parts = [label_rows(src[a:a + chunk_rows], **p) for a in range(0, src.shape[0], chunk_rows)]
    out = torch.cat(parts, dim=0) if parts else torch.empty(0, p["n_beams"] + 1, dtype=torch.float32, device=src.device)
    return DeviceDataset.from_tensor(out)
