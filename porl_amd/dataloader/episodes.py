"""Episode tables, the return range and hindsight-goal batches on the device — the trajectory-level dataset functions
of the reference (util/util.py:67-138) on resident rows (csrc/episodes.hpp):

    extract_done_makers(dones)                  -> (starts, ends, lengths)            util/util.py:83-87
    episode_returns(rewards, terminals, cap)    -> (returns fp64 (K,), lengths int64 (K+1,))   the two lists of :67-80
    return_range(dataset, max_episode_steps)    -> (min, max) as Python floats        util/util.py:67-80
    hindsight_indices(index, batch_size, ...)   -> (start, goal) int64                util/util.py:90-116
    gather_pairs(rows, start, goal, S, A)       -> packed (B, 2S+2+A) batch
    rvs_sample_batch(replay, batch_size)        -> dict of batch tensors              util/util.py:129-138

A done flag is set iff it is != 0.0 (NaN counts as set, -0.0 as clear, like `np.where(dones)` and `if d`).  Flags and
rewards may be strided views — column 2S+1 / S of a packed row store is read in place, nothing is copied.

`EpisodeIndex` is the table of a row store: one count pass, ONE read-back of the episode count (the only
synchronisation, once per dataset), one fill pass.  Everything after it — the draw, the gather — stays on the device.

Data-parallel shards: the table is that of the rank's LOCAL rows.  A trajectory cut by the shard boundary contributes
its tail as an episode that starts at local row 0; its head is the previous rank's trailing, unterminated run and is
dropped there, exactly as the reference drops the trailing trajectory of the whole dataset.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _native as N

_tiles = None


def tile_constants():
    """(rows per block, partials per sweep) of the episode scan — the sizes at which its code path changes."""
    global _tiles
    if _tiles is None:
        t, p = C.c_int32(0), C.c_int32(0)
        N.lib().porl_episode_workspace(1, C.byref(t), C.byref(p))
        _tiles = (int(t.value), int(p.value))
    return _tiles


def _vector(x, name):
    """(base tensor, stride in floats, n) of a (N,) fp32 device view."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: expected a torch tensor, got {type(x).__name__}")
    if x.device.type != "cuda":
        raise N.NativeError(f"{name}: the episode passes run on a HIP device only (no CPU path)")
    if x.dim() != 1 or x.dtype != torch.float32:
        raise ValueError(f"{name}: expected (N,) float32, got {x.dtype} {tuple(x.shape)}")
    n = x.shape[0]
    stride = x.stride(0) if n > 1 else 1           # the stride of a one-element view is arbitrary
    if n > 1 and stride < 1:
        raise ValueError(f"{name}: stride {stride} (an expanded or reversed view cannot be read in place)")
    return x, stride, n


def _rows_of(store):
    return store.rows if hasattr(store, "rows") else store


def episode_table(flags, cap):
    """(starts, ends, trailing) of the closed episodes of a flag vector; cap 0 = none."""
    flags, stride, n = _vector(flags, "dones")
    dev = flags.device
    if n == 0:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return e, e.clone(), 0
    lib = N.lib()
    words = lib.porl_episode_workspace(n, None, None)
    if words < 0:
        N.check(-1, "porl_episode_workspace")
    ws = torch.empty(words, dtype=torch.int64, device=dev)
    stream = N.current_stream_ptr(flags)
    N.check(lib.porl_episode_count(N.ptr(flags), stride, n, cap, N.ptr(ws), stream), "porl_episode_count")
    k, trailing = ws[:2].tolist()                  # the one read-back
    starts = torch.empty(k, dtype=torch.int64, device=dev)
    ends = torch.empty(k, dtype=torch.int64, device=dev)
    if k > 0:
        N.check(lib.porl_episode_fill(N.ptr(flags), stride, n, cap, N.ptr(ws), k, N.ptr(starts), N.ptr(ends), stream),
                "porl_episode_fill")
    return starts, ends, int(trailing)


class EpisodeIndex:
    """The episode table of a row store: `starts`, `ends`, `lengths` (int64 device tensors of `n_episodes` entries),
    `n_rows`, and `trailing`, the rows after the last set flag, which belong to no episode.  With no set flag the table
    is empty (the reference returns starts = [0] there and its only caller then raises IndexError)."""

    def __init__(self, starts, ends, n_rows, trailing):
        self.starts, self.ends = starts, ends
        self.lengths = ends - starts + 1
        self.n_rows, self.trailing = int(n_rows), int(trailing)
        self.n_episodes = int(starts.numel())

    @classmethod
    def from_dones(cls, dones):
        """From any (N,) fp32 device view of done flags, a strided column included."""
        starts, ends, trailing = episode_table(dones, 0)
        return cls(starts, ends, dones.shape[0], trailing)

    @classmethod
    def from_replay(cls, store, obs_dim=None, timeouts=None):
        """From a PackedReplay / DeviceDataset / (N, width) row tensor: the flags are `timeouts` when given
        (util/util.py:91-94), else column 2*obs_dim + 1 of the rows, read in place.  `obs_dim` defaults to the store's.
        On a data-parallel shard this is the table of the local rows (see the module docstring)."""
        if timeouts is not None:
            return cls.from_dones(timeouts)
        rows = _rows_of(store)
        S = getattr(store, "obs_dim", None) if obs_dim is None else obs_dim
        if S is None:
            raise ValueError("obs_dim: the store does not carry one, pass it")
        if rows.dim() != 2 or rows.shape[1] < 2 * S + 2:
            raise ValueError(f"rows {tuple(rows.shape)} have no done column 2*{S}+1")
        if rows.device.type != "cuda":
            raise N.NativeError("EpisodeIndex.from_replay: the rows are not on a HIP device (no CPU path)")
        return cls.from_dones(rows[:, 2 * S + 1])

    def __len__(self):
        return self.n_episodes


def extract_done_makers(dones):
    """util/util.py:83-87: (starts, ends, lengths), int64 device tensors.  Empty when no flag is set."""
    ix = EpisodeIndex.from_dones(dones)
    return ix.starts, ix.ends, ix.lengths


def _returns(rewards, terminals, max_episode_steps, want_range):
    if max_episode_steps is None or int(max_episode_steps) != max_episode_steps or max_episode_steps < 1:
        raise ValueError(f"max_episode_steps {max_episode_steps!r}: need an integer >= 1")
    rewards, r_stride, n = _vector(rewards, "rewards")
    terminals, _, nt = _vector(terminals, "terminals")
    if nt != n:
        raise ValueError(f"rewards ({n}) and terminals ({nt}) differ in length")
    if terminals.device != rewards.device:
        raise ValueError("rewards and terminals live on different devices")
    starts, ends, trailing = episode_table(terminals, int(max_episode_steps))
    dev = rewards.device
    k = starts.numel()
    returns = torch.empty(k, dtype=torch.float64, device=dev)
    lengths = torch.cat([ends - starts + 1, torch.tensor([trailing], dtype=torch.int64, device=dev)])
    rng = None
    if k > 0:
        ws = torch.empty(4 * 256, dtype=torch.int64, device=dev) if want_range else None
        rng = torch.empty(3, dtype=torch.float64, device=dev) if want_range else None
        N.check(N.lib().porl_episode_returns(N.ptr(rewards), r_stride, n, N.ptr(starts), N.ptr(ends), k, N.ptr(returns),
                                             N.ptr(ws), N.ptr(rng), N.current_stream_ptr(rewards)), "porl_episode_returns")
    return returns, lengths, rng


def episode_returns(rewards, terminals, max_episode_steps):
    """The two lists return_range builds (util/util.py:68-78): `returns` (K,) fp64 — per closed episode the sum of its
    fp32 rewards added in row order as a Python float would — and `lengths` (K+1,) int64, whose last entry is the
    trailing, unclosed run (it sums to N with the others).  An episode closes at a set terminal or after
    `max_episode_steps` rows."""
    returns, lengths, _ = _returns(rewards, terminals, max_episode_steps, False)
    return returns, lengths


def return_range(dataset, max_episode_steps):
    """util/util.py:67-80: (min, max) episode return as Python floats.  `dataset` is a dict with 'rewards' and
    'terminals' device tensors (the reference's signature) or a PackedReplay (columns S and 2S+1, read in place).

    Raises ValueError where the reference does (no closed episode: min() of an empty list), for max_episode_steps < 1
    (no sensible reading upstream), and when an episode return is NaN: the reference's answer then depends on WHERE the
    NaN episode sits in the list (min / max keep whichever operand makes the comparison false), so there is no value to
    reproduce."""
    if isinstance(dataset, dict):
        rewards, terminals = dataset["rewards"], dataset["terminals"]
    else:
        rows, S = _rows_of(dataset), dataset.obs_dim
        if rows.device.type != "cuda":
            raise N.NativeError("return_range: the rows are not on a HIP device (no CPU path)")
        rewards, terminals = rows[:, S], rows[:, 2 * S + 1]
    returns, _, rng = _returns(rewards, terminals, max_episode_steps, True)
    if returns.numel() == 0:
        raise ValueError("return_range: no closed episode (min() arg is an empty sequence)")
    lo, hi, saw_nan = rng.tolist()
    if saw_nan != 0.0:
        raise ValueError("return_range: an episode return is NaN; the reference's min / max then depend on its position")
    return lo, hi


def hindsight_indices(index, batch_size, seed=0, step=0, *, traj=None, u1=None, u2=None, return_draws=False):
    """util/util.py:90-116 on an EpisodeIndex: (start, goal) int64 (B,), a row and a later (or the same) row of one
    trajectory; with `return_draws` also the (traj, u1, u2) used.  The draws are a counter-based stream keyed by
    (seed, step) — the same key gives the same batch — unless `traj` (int64), `u1`, `u2` (fp64 in [0, 1)) are given.
    Raises IndexError on an empty table, the reference's exception."""
    if index.starts.device.type != "cuda":
        raise N.NativeError("hindsight_indices: the episode table is not on a HIP device (no CPU path)")
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size} must be positive")
    if index.n_episodes < 1:
        raise IndexError("hindsight_indices: the dataset has no closed episode")
    dev = index.starts.device
    given = [traj, u1, u2]
    if any(g is not None for g in given):
        if any(g is None for g in given):
            raise ValueError("traj, u1 and u2 are given together or not at all")
        for g, dt, name in ((traj, torch.int64, "traj"), (u1, torch.float64, "u1"), (u2, torch.float64, "u2")):
            if g.device != dev:
                raise N.NativeError(f"{name}: not on the table's device (no CPU path)")
            if g.dtype != dt or g.shape != (batch_size,) or not g.is_contiguous():
                raise ValueError(f"{name}: expected a contiguous ({batch_size},) {dt} tensor")
    start = torch.empty(batch_size, dtype=torch.int64, device=dev)
    goal = torch.empty(batch_size, dtype=torch.int64, device=dev)
    d_traj = torch.empty(batch_size, dtype=torch.int64, device=dev) if return_draws else None
    d_u1 = torch.empty(batch_size, dtype=torch.float64, device=dev) if return_draws else None
    d_u2 = torch.empty(batch_size, dtype=torch.float64, device=dev) if return_draws else None
    mask = 0xFFFFFFFFFFFFFFFF
    N.check(N.lib().porl_hindsight_pairs(N.ptr(index.starts), N.ptr(index.lengths), index.n_episodes, batch_size, seed & mask,
                                         step & mask, N.ptr(traj), N.ptr(u1), N.ptr(u2), N.ptr(start), N.ptr(goal), N.ptr(d_traj),
                                         N.ptr(d_u1), N.ptr(d_u2), N.current_stream_ptr(start)), "porl_hindsight_pairs")
    return (start, goal, d_traj, d_u1, d_u2) if return_draws else (start, goal)


def gather_pairs(rows, start, goal, obs_dim, act_dim, out=None):
    """Packed hindsight batch (B, 2S+2+A): `[ rows[start][:S] | 0 | rows[goal][:S] | 0 | rows[start][2S+2:] ]` — the wire
    format of PackedReplay, so `PackedReplay.split` and the agents' strided-view inputs work unchanged.  `rows` may be
    a strided view with unit column stride."""
    if rows.device.type != "cuda":
        raise N.NativeError("gather_pairs: the rows are not on a HIP device (no CPU path)")
    W = 2 * obs_dim + 2 + act_dim
    if rows.dim() != 2 or rows.dtype != torch.float32 or rows.shape[1] < W or rows.shape[0] < 1:
        raise ValueError(f"rows: expected (N >= 1, >= {W}) float32, got {rows.dtype} {tuple(rows.shape)}")
    if rows.shape[1] > 1 and rows.stride(1) != 1:
        raise ValueError("rows must have unit column stride")
    B = start.numel()
    for t, name in ((start, "start"), (goal, "goal")):
        if t.device != rows.device or t.dtype != torch.int64 or t.dim() != 1 or t.numel() != B or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous (B,) int64 tensor on the rows' device")
    if out is None:
        out = torch.empty(B, W, dtype=torch.float32, device=rows.device)
    elif out.shape != (B, W) or out.dtype != torch.float32 or out.device != rows.device or out.stride(1) != 1:
        raise ValueError(f"out: expected ({B}, {W}) float32 on the rows' device with unit column stride")
    n = rows.shape[0]
    stride = rows.stride(0) if n > 1 else max(rows.stride(0), W)
    out_stride = out.stride(0) if B > 1 else max(out.stride(0), W)
    N.check(N.lib().porl_gather_pairs(N.ptr(rows), stride, n, N.ptr(start), N.ptr(goal), B, obs_dim, act_dim, N.ptr(out),
                                      out_stride, N.current_stream_ptr(rows)), "porl_gather_pairs")
    return out


def rvs_sample_batch(replay, batch_size, index=None):
    """util/util.py:129-138 on a PackedReplay: observations and actions of row `start`, next_observations = the
    observation of row `goal`, a later row of the same trajectory.  The draw is keyed by (replay.seed, replay.draws) and
    `replay.draws` advances by one per call, as `sample_indices` does.  The episode table is built on the first call and
    cached on the replay (pass `index` to use another, e.g. one built from timeouts).

    Deviation: `rewards` and `terminals` are (B,) zero tensors — the zero columns of the packed batch — where the
    reference stores the Python int 0, which its own agents cannot consume (`terminals.float()` fails on an int).  The
    values are views of one packed batch buffer that the next call with the same batch size overwrites, like
    `PackedReplay.sample`."""
    rows = replay.rows
    if rows.device.type != "cuda":
        raise N.NativeError("rvs_sample_batch: the replay store is not on a HIP device (no CPU path)")
    if index is None:
        index = getattr(replay, "_episode_index", None)
        if index is None:
            index = replay._episode_index = EpisodeIndex.from_replay(replay)
    start, goal = hindsight_indices(index, batch_size, seed=replay.seed, step=replay.draws)
    replay.draws += 1
    S, A = replay.obs_dim, replay.act_dim
    out = getattr(replay, "_pair_out", None)
    if out is None or out.shape[0] != batch_size:
        out = replay._pair_out = torch.empty(batch_size, 2 * S + 2 + A, dtype=torch.float32, device=rows.device)
    batch = gather_pairs(rows, start, goal, S, A, out=out)
    obs, rew, nxt, term, act = replay.split(batch)
    return {"observations": obs, "actions": act, "next_observations": nxt, "rewards": rew, "terminals": term}
