"""Hold out a region of a resident dataset — the reference's `generate_test_generlaization_data`
(util/util.py:219-238) on the device (csrc/partition.hpp):

    partition_rows(store_or_tensor, held | x_range, y_range)   -> Partition: one buffer, kept rows first, held rows behind
    holdout_region(replay, env_name | x_range, y_range)        -> (train, held), two PackedReplay over that buffer
    generate_test_generlaization_data(dataset, env_name)       the reference's signature (its spelling), on a dict of
                                                               device tensors; also re-exported from porl_amd.util.util

The reference deletes every transition whose first two observation coordinates lie in a fixed box, so that an agent can
be trained without a region of the maze and tested on it; the deleted rows are lost.  Here the store is copied ONCE into
a buffer of the same size, rows outside the box first and rows inside it behind them, each part in input order, and both
parts are views of that buffer.  The box test is made in fp32 with both ends inclusive; a NaN coordinate is not in the
box (numpy's comparisons).  Rows travel as raw 32-bit words: NaN payloads and -0.0 survive.

One read-back per call (the number of kept rows, to cut the two views) is the only synchronisation.

Deviations, both upstream's own behaviour kept: rows are deleted from the MIDDLE of trajectories, so an `EpisodeIndex`
built on either part splices what is left of a trajectory to its neighbours (a run of rows between two done flags may
mix several visits to the region's border) — build the episode table on the whole store when trajectories matter.  On
a data-parallel shard everything acts on the rank's local rows.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native as N

# util/util.py:220-227: (substring of the env name, x range, y range) tried in order; None matches every name
HOLDOUT_BOXES = (("umaze", (5, 10), (2, 7)), ("medium", (10, 15), (10, 15)), (None, (26, 30), (14, 18)))

_tiles = None


def tile_constants():
    """(rows per block, partials per sweep) of the partition — the sizes at which its code path changes."""
    global _tiles
    if _tiles is None:
        t, p = C.c_int32(0), C.c_int32(0)
        N.lib().porl_partition_workspace(1, C.byref(t), C.byref(p))
        _tiles = (int(t.value), int(p.value))
    return _tiles


def box_for(env_name):
    """(x_range, y_range) the reference deletes for `env_name` (util/util.py:220-227)."""
    for key, xr, yr in HOLDOUT_BOXES:
        if key is None or key in env_name:
            return xr, yr
    raise AssertionError("HOLDOUT_BOXES ends with a catch-all")


class Partition:
    """`rows` (N, W): the kept rows, then the held rows, each in input order; `n_kept`; the views `kept` = rows[:n_kept]
    and `held` = rows[n_kept:]; `index` (int64 (N,), or None): the original row number of every output row."""

    def __init__(self, rows, n_kept, index=None):
        self.rows, self.n_kept, self.index = rows, int(n_kept), index

    @property
    def kept(self):
        return self.rows[:self.n_kept]

    @property
    def held(self):
        return self.rows[self.n_kept:]


def _as_rows(x, name="rows"):
    """The (N, W) view to partition: the rows of a store, a 2-D tensor with unit column stride, or a vector as (N, 1)."""
    t = x.rows if hasattr(x, "rows") else x
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a PackedReplay, a DeviceDataset or a torch tensor, got {type(x).__name__}")
    if t.element_size() not in (4, 8) or t.dtype == torch.bool or t.is_complex():
        raise TypeError(f"{name}: rows are copied as 32-bit words, need a 4- or 8-byte dtype, got {t.dtype}")
    if t.device.type != "cuda":
        raise N.NativeError(f"{name}: the partition runs on a HIP device only (no CPU path)")
    if t.dim() == 1:
        t = t.unsqueeze(1)
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError(f"{name}: expected (N, W >= 1) or (N,), got {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: rows must have unit column stride")
    if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        raise ValueError(f"{name}: row stride {t.stride(0)} (an expanded or overlapping view cannot be read in place)")
    return t


def _box(t, x_range, y_range, cols):
    if t.dtype != torch.float32:
        raise TypeError(f"the box is tested on fp32 columns, the rows are {t.dtype}")
    cx, cy = (int(c) for c in cols)
    if not (0 <= cx < t.shape[1] and 0 <= cy < t.shape[1]):
        raise ValueError(f"cols {tuple(cols)} outside the row's {t.shape[1]} columns")
    (x_lo, x_hi), (y_lo, y_hi) = x_range, y_range
    return N.PartitionBox(cx, cy, float(x_lo), float(x_hi), float(y_lo), float(y_hi))   # c_float rounds to fp32


def _strides(t):
    item, (n, w) = t.element_size(), t.shape
    row_bytes = w * item
    return (t.stride(0) * item if n > 1 else row_bytes), row_bytes


def _launch(t, held, box, want_index):
    """Queue one partition of the (N >= 1, W) view `t`; -> (out, index, workspace), nothing read back."""
    n = t.shape[0]
    dev = t.device
    lib = N.lib()
    words = lib.porl_partition_workspace(n, None, None)
    if words < 0:
        N.check(-1, "porl_partition_workspace")
    ws = torch.empty(words, dtype=torch.int64, device=dev)
    out = torch.empty(t.shape, dtype=t.dtype, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev) if want_index else None
    stride_bytes, row_bytes = _strides(t)
    N.check(lib.porl_partition_rows(N.ptr(t), stride_bytes, n, row_bytes, N.ptr(held), None if box is None else C.byref(box),
                                    N.ptr(out), N.ptr(index), N.ptr(ws), N.current_stream_ptr(t)), "porl_partition_rows")
    return out, index, ws


def _held_vector(held, t):
    if not isinstance(held, torch.Tensor):
        raise TypeError(f"held: expected a torch tensor, got {type(held).__name__}")
    if held.device != t.device:
        raise N.NativeError("held: not on the rows' device (no CPU path)")
    if held.dtype == torch.bool:
        held = held.view(torch.uint8)
    if held.dtype != torch.uint8 or held.shape != (t.shape[0],):
        raise ValueError(f"held: expected a ({t.shape[0]},) uint8 or bool tensor, got {held.dtype} {tuple(held.shape)}")
    return held.contiguous()


def partition_rows(store_or_tensor, held=None, *, x_range=None, y_range=None, cols=(0, 1), return_index=False):
    """Stable two-way partition -> `Partition`.  The predicate is EITHER `held`, a (N,) uint8 / bool device vector
    (nonzero = held), OR the box `x_range[0] <= row[cols[0]] <= x_range[1] and y_range[0] <= row[cols[1]] <= y_range[1]`
    on two fp32 columns, evaluated inside the kernels (bounds rounded to fp32, NaN coordinates kept).

    Accepts a PackedReplay, a DeviceDataset, or an (N, W) / (N,) tensor of a 4- or 8-byte dtype with unit column stride;
    a row-strided view or a column block of a wider tensor is read in place, never copied first, never written.  Other
    dtypes raise TypeError, a CPU tensor NativeError."""
    t = _as_rows(store_or_tensor)
    ranges = x_range is not None or y_range is not None
    if (held is not None) == ranges or (ranges and (x_range is None or y_range is None)):
        raise ValueError("give exactly one of `held` and the pair `x_range`, `y_range`")
    box = _box(t, x_range, y_range, cols) if ranges else None
    mask = _held_vector(held, t) if held is not None else None
    if t.shape[0] == 0:
        return Partition(t.clone(), 0, torch.empty(0, dtype=torch.int64, device=t.device) if return_index else None)
    out, index, ws = _launch(t, mask, box, return_index)
    n_kept = int(ws[0])                                # the one read-back
    if hasattr(store_or_tensor, "dim") and store_or_tensor.dim() == 1:
        out = out.view(-1)
    return Partition(out, n_kept, index)


def _mix(seed, salt):
    """splitmix64's output function on seed ^ salt * golden ratio: the two parts draw different streams."""
    m = 0xFFFFFFFFFFFFFFFF
    z = ((seed ^ (salt * 0x9E3779B97F4A7C15)) + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def holdout_region(replay, env_name=None, *, x_range=None, y_range=None, cols=(0, 1)):
    """(train, held): two PackedReplay over the two views of ONE partitioned copy of `replay.rows` — the rows outside
    the box and the rows inside it.  The box is the reference's for `env_name` (`HOLDOUT_BOXES`) or the given ranges.
    Both parts carry the source's obs_dim / act_dim, start at draws = 0 and draw streams of their own derived from the
    source's seed.  See the module docstring for what happens to trajectories and shards."""
    from ..buffer.replay_buffer import PackedReplay
    if (env_name is None) == (x_range is None and y_range is None):
        raise ValueError("give exactly one of `env_name` and the pair `x_range`, `y_range`")
    if env_name is not None:
        x_range, y_range = box_for(env_name)
    part = partition_rows(replay, x_range=x_range, y_range=y_range, cols=cols)
    out = []
    for salt, rows in ((1, part.kept), (2, part.held)):
        r = PackedReplay(rows, replay.obs_dim, replay.act_dim, rows.device)
        r.seed = _mix(replay.seed, salt)
        out.append(r)
    return tuple(out)


def generate_test_generlaization_data(dataset, env_name, env_idx=None):
    """util/util.py:219-238 (the reference's spelling) on a dict of device tensors with a common first dimension: every
    row whose `dataset["observations"][:, :2]` lies in the box of `env_name` is deleted from every value.  The dict is
    updated in place and returned; `env_idx` is accepted and ignored, as upstream.  One mask launch, one partition per
    key, one read-back.  The new values are the leading views of the partition buffers.  Values need a 4- or 8-byte
    dtype (convert bool flags first).  For a PackedReplay it returns the `train` part of `holdout_region`."""
    if not isinstance(dataset, dict):
        return holdout_region(dataset, env_name)[0]
    x_range, y_range = box_for(env_name)
    obs = _as_rows(dataset["observations"], "observations")
    n = obs.shape[0]
    views = {k: _as_rows(v, k) for k, v in dataset.items()}
    for k, t in views.items():
        if t.shape[0] != n or t.device != obs.device:
            raise ValueError(f"{k}: {t.shape[0]} rows on {t.device}, observations have {n} on {obs.device}")
    if n == 0:
        return dataset
    box = _box(obs, x_range, y_range, (0, 1))
    mask = torch.empty(n, dtype=torch.uint8, device=obs.device)
    stride_bytes, row_bytes = _strides(obs)
    N.check(N.lib().porl_partition_mask(N.ptr(obs), stride_bytes, n, row_bytes, C.byref(box), N.ptr(mask),
                                        N.current_stream_ptr(obs)), "porl_partition_mask")
    outs = {k: _launch(t, mask, None, False) for k, t in views.items()}
    n_kept = int(next(iter(outs.values()))[2][0])      # the one read-back
    for k, (out, _, _) in outs.items():
        dataset[k] = out[:n_kept].view(-1) if dataset[k].dim() == 1 else out[:n_kept]
    return dataset
