"""Normalise a resident dataset — the reference's `--normalize` (por_train.py:141, sorl_train.py:95) on the device
(csrc/colstats.hpp):

    column_stats(store_or_rows, cols=None)            -> ColumnStats: n, mean, m2, min, max per column, host fp64
    Normalizer(mean, std, reward_div, reward_mul)     .from_stats / .with_reward_scale / .apply / .apply_ / state_dict
    normalize_dataset(replay, max_episode_steps=None) -> Normalizer; the store's s, s' (and r) columns rewritten in place

The reference's evaluators compute `obs = (obs - mean) / std` before every `policy.act` (util/util.py:146,160,177) from
the dataset's `mean, std`, and its `return_range` (:67-80) exists to rescale rewards, `r /= (max_ret - min_ret);
r *= max_episode_steps`.  Here the statistics are ONE deterministic fp64 pass over the rows where they lie (a dense
store, a row-strided view, either part of a `holdout_region`), and the three rewrites are ONE in-place sweep: columns
[0, S) and [S+1, 2S+1) by the same mean / std, column S by the reward scale.  Every element becomes
fl(fl(x - mean) / std) — two IEEE fp32 operations, the quotient a true division — and a reward fl(fl(r / div) * mul),
which is what numpy computes for the reference's expressions on fp32 arrays.

Statistics are taken from the observation columns only, never from the next observations (upstream).  `std` is the
population one (numpy's ddof = 0) plus `eps`.  On a data-parallel shard everything acts on the rank's local rows;
`ColumnStats.merge` combines shard statistics on the host (wiring it into torch.distributed is the caller's).

One read-back of 4 * C doubles per `column_stats` is the only synchronisation.  There is no CPU path.

A store that feeds a FasterNet backbone must stay RAW: `state2costmap` reads its range columns in metres.  Nothing here
enforces that.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _native as N

_tiles = None


def tile_constants():
    """(rows per block, partials per sweep) of the statistics pass — the sizes at which its code path changes."""
    global _tiles
    if _tiles is None:
        t, p = C.c_int32(0), C.c_int32(0)
        N.lib().porl_colstats_workspace(1, 1, C.byref(t), C.byref(p))
        _tiles = (int(t.value), int(p.value))
    return _tiles


def _as_rows(x, name="rows"):
    """The (N, W) fp32 device view of a store or tensor; a vector counts as (1, W) for `Normalizer.apply`'s callers."""
    t = x.rows if hasattr(x, "rows") else x
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a PackedReplay, a DeviceDataset or a torch tensor, got {type(x).__name__}")
    if t.device.type != "cuda":
        raise N.NativeError(f"{name}: the normalisation passes run on a HIP device only (no CPU path)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32 rows, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError(f"{name}: expected (N, W >= 1), got {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: rows must have unit column stride")
    if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        raise ValueError(f"{name}: row stride {t.stride(0)} (an expanded or overlapping view cannot be used in place)")
    return t


def _stride(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def col_stats_device(t, col0, n_cols):
    """Queue the statistics of columns [col0, col0 + n_cols) of the (N >= 1, W) view `t`; -> (4, n_cols) fp64 device
    tensor [mean | M2 | min | max], nothing read back."""
    n, w = t.shape
    col0, n_cols = int(col0), int(n_cols)
    if n < 1:
        raise ValueError("column statistics of no rows")
    if n_cols < 1 or col0 < 0 or col0 + n_cols > w:
        raise ValueError(f"cols ({col0}, {n_cols}) outside the row's {w} columns")
    lib = N.lib()
    words = lib.porl_colstats_workspace(n, n_cols, None, None)
    if words < 0:
        N.check(-1, "porl_colstats_workspace")
    ws = torch.empty(words, dtype=torch.float64, device=t.device)
    out = torch.empty(4, n_cols, dtype=torch.float64, device=t.device)
    N.check(lib.porl_col_stats(N.ptr(t), _stride(t), n, col0, n_cols, N.ptr(ws), N.ptr(out), N.current_stream_ptr(t)),
            "porl_col_stats")
    return out


def affine_cols_device(t, spans, shift, div, mul=None, out=None):
    """Queue out[:, c0+j] = fl(fl(t[:, c0+j] - shift[p0+j]) / div[p0+j]) [* mul[p0+j] with flag 1] for every span
    (c0, n_cols, p0, flags); out defaults to `t` itself (in place), else it is an fp32 view of the same rows and at least
    as many columns that shares no element with `t`.  Nothing is read back."""
    n, w = t.shape
    if out is None:
        out = t
    else:
        out = _as_rows(out, "out")
        if out.device != t.device or out.shape[0] != n or out.shape[1] < w:
            raise ValueError(f"out: expected ({n}, >= {w}) on {t.device}, got {tuple(out.shape)} on {out.device}")
        same = out.data_ptr() == t.data_ptr() and _stride(out) == _stride(t)
        if not same and n > 0:                                      # element (i, c) of one buffer under (i', c') of the other
            lo_t, lo_o = t.data_ptr(), out.data_ptr()
            hi_t = lo_t + 4 * ((n - 1) * _stride(t) + w)
            hi_o = lo_o + 4 * ((n - 1) * _stride(out) + w)
            st, off = _stride(t), (lo_o - lo_t) // 4
            blocks = _stride(out) == st and w <= off % st <= st - w  # two column blocks of one pitch never meet
            if lo_t < hi_o and lo_o < hi_t and not blocks:
                raise ValueError("out: partly overlaps the rows (use the rows themselves for an in-place pass)")
    if n == 0:
        return out
    arr = (N.ColSpan * len(spans))(*[N.ColSpan(*(int(v) for v in s)) for s in spans])
    for name, v in (("shift", shift), ("div", div), ("mul", mul)):
        if v is not None and (v.device != t.device or v.dtype != torch.float32 or v.dim() != 1 or not v.is_contiguous()
                              or v.numel() != shift.numel()):
            raise ValueError(f"{name}: expected a contiguous float32 vector of {shift.numel()} entries on {t.device}")
    N.check(N.lib().porl_affine_cols(N.ptr(t), _stride(t), n, w, arr, len(spans), N.ptr(shift), N.ptr(div), N.ptr(mul),
                                     shift.numel(), N.ptr(out), _stride(out), N.current_stream_ptr(t)), "porl_affine_cols")
    return out


def _merge(a, b):
    """The pairwise update on host arrays: (n, mean, m2, min, max) of the union of two disjoint samples."""
    na, ma, sa, lo_a, hi_a = a
    nb, mb, sb, lo_b, hi_b = b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    with np.errstate(invalid="ignore", over="ignore"):
        r = nb / n
        d = mb - ma
        return n, ma + d * r, sa + sb + d * d * (na * r), np.minimum(lo_a, lo_b), np.maximum(hi_a, hi_b)


class ColumnStats:
    """Host numpy fp64 statistics of C columns over `n` rows: `mean`, `m2` = sum (x - mean)^2, `min`, `max`;
    `var` = m2 / n (population, numpy's ddof = 0) and `std`.  `device` is where the rows lay (None when built by hand)."""

    def __init__(self, n, mean, m2, min, max, device=None):
        self.n = int(n)
        self.mean, self.m2, self.min, self.max = (np.array(v, dtype=np.float64).reshape(-1) for v in (mean, m2, min, max))
        self.device = device

    @property
    def var(self):
        with np.errstate(invalid="ignore"):
            return self.m2 / self.n

    @property
    def std(self):
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.var)

    def merge(self, *others):
        """The statistics of this sample and `others` together (disjoint rows, the same columns), combined left to
        right by the update the kernels use: d = mean_b - mean_a, mean = mean_a + d n_b / n,
        m2 = m2_a + m2_b + d^2 n_a n_b / n.  Returns a new ColumnStats."""
        acc = (self.n, self.mean, self.m2, self.min, self.max)
        for o in others:
            if o.mean.shape != self.mean.shape:
                raise ValueError(f"merge: {o.mean.shape[0]} columns against {self.mean.shape[0]}")
            acc = _merge(acc, (o.n, o.mean, o.m2, o.min, o.max))
        return ColumnStats(*acc, device=self.device)


def column_stats(store_or_rows, cols=None):
    """Per-column statistics of a PackedReplay, a DeviceDataset or any (N, W) fp32 device view with unit column stride
    (row-strided views and column blocks are read in place, never copied, never written).  `cols` = (col0, n_cols);
    default: the observation columns (0, obs_dim) of a store that carries `obs_dim`, else every column.  fp64
    throughout, deterministic: equal values give equal bits whatever the view (dense, row-strided, any col0) for the
    same n_cols; the combine order depends on n_rows and n_cols, so a column taken inside a wider span agrees to
    rounding, not bit for bit.  A NaN in a column gives NaN in its four results (numpy's mean / min / max)."""
    t = _as_rows(store_or_rows)
    if cols is None:
        S = getattr(store_or_rows, "obs_dim", None)
        cols = (0, t.shape[1] if S is None else S)
    col0, n_cols = cols
    out = col_stats_device(t, col0, n_cols).cpu().numpy()          # the one read-back
    return ColumnStats(t.shape[0], out[0], out[1], out[2], out[3], device=t.device)


class Normalizer:
    """`mean`, `std`: fp32 (S,) vectors; `reward_div`, `reward_mul`: fp32-representable floats or None.
    x -> fl(fl(x - mean) / std);  r -> fl(fl(r / reward_div) * reward_mul)."""

    def __init__(self, mean, std, reward_div=None, reward_mul=None):
        mean, std = (torch.as_tensor(v, dtype=torch.float32).reshape(-1).contiguous() for v in (mean, std))
        if mean.shape != std.shape or mean.numel() < 1:
            raise ValueError(f"mean {tuple(mean.shape)} and std {tuple(std.shape)}: expected two (S >= 1,) vectors")
        if mean.device != std.device:
            raise ValueError("mean and std live on different devices")
        self.mean, self.std = mean, std
        self.reward_div = None if reward_div is None else float(np.float32(reward_div))
        self.reward_mul = None if reward_mul is None else float(np.float32(reward_mul))
        if (self.reward_div is None) != (self.reward_mul is None):
            raise ValueError("reward_div and reward_mul come together")
        self._packed = None

    @property
    def obs_dim(self):
        return self.mean.numel()

    @property
    def device(self):
        return self.mean.device

    @classmethod
    def from_stats(cls, stats, eps=1e-3, device=None):
        """mean32 = fp32(mean64), std32 = fp32(sqrt(m2 / n) + eps), computed on the host.  A non-finite value raises
        ValueError naming the column."""
        with np.errstate(invalid="ignore", over="ignore"):
            mean32 = stats.mean.astype(np.float32)
            std32 = (np.sqrt(stats.m2 / stats.n) + eps).astype(np.float32)
        bad = np.flatnonzero(~(np.isfinite(mean32) & np.isfinite(std32)))
        if bad.size:
            c = int(bad[0])
            raise ValueError(f"column {c}: mean {mean32[c]} / std {std32[c]} is not finite "
                             f"({bad.size} such column{'s' if bad.size > 1 else ''}: {bad[:8].tolist()})")
        device = device if device is not None else (stats.device if stats.device is not None else "cpu")
        return cls(torch.from_numpy(mean32).to(device), torch.from_numpy(std32).to(device))

    def with_reward_scale(self, lo, hi, max_episode_steps):
        """r /= (hi - lo); r *= max_episode_steps — (lo, hi) = return_range of the RAW rewards.  Returns self."""
        if hi == lo:
            raise ValueError(f"reward scale: max return == min return == {lo} (the reference divides by zero here)")
        div, mul = np.float32(float(hi) - float(lo)), np.float32(max_episode_steps)
        if not (np.isfinite(div) and np.isfinite(mul)):
            raise ValueError(f"reward scale: ({lo}, {hi}, {max_episode_steps}) is not finite in fp32")
        self.reward_div, self.reward_mul = float(div), float(mul)
        self._packed = None
        return self

    def to(self, device):
        self.mean, self.std = self.mean.to(device), self.std.to(device)
        self._packed = None
        return self

    def _params(self):
        """(shift, div, mul) device vectors of S + 1 entries: the observation parameters, then the reward's."""
        if self._packed is None:
            one = self.mean.new_ones(1)
            shift = torch.cat([self.mean, one * 0])
            div = torch.cat([self.std, one * (1.0 if self.reward_div is None else self.reward_div)])
            mul = torch.cat([torch.ones_like(self.mean), one * (1.0 if self.reward_mul is None else self.reward_mul)])
            self._packed = (shift, div, mul)
        return self._packed

    def _on(self, t, what):
        if self.mean.device != t.device:
            raise ValueError(f"{what}: the rows are on {t.device}, the normalizer on {self.mean.device} (use .to)")

    def apply(self, obs, out=None):
        """(B, S) or (S,) device observations -> a new normalised tensor (or `out`); a strided view is read in place,
        the input is not written."""
        squeeze = isinstance(obs, torch.Tensor) and obs.dim() == 1
        t = _as_rows(obs.unsqueeze(0) if squeeze else obs, "obs")
        S = self.obs_dim
        if t.shape[1] != S:
            raise ValueError(f"obs: {t.shape[1]} columns, the normalizer has {S}")
        self._on(t, "obs")
        if out is None:
            res = torch.empty(t.shape, dtype=torch.float32, device=t.device)
        else:
            res = _as_rows(out.unsqueeze(0) if out.dim() == 1 else out, "out")
            if res.shape != t.shape or res.device != t.device:
                raise ValueError(f"out: expected {tuple(t.shape)} on {t.device}")
        affine_cols_device(t, [(0, S, 0, 0)], self.mean, self.std, None, out=res)
        return out if out is not None else (res[0] if squeeze else res)

    def apply_(self, store_or_rows):
        """Normalise columns [0, S) and [S+1, 2S+1) of a packed [s | r | s' | d | a] store in place, by the same
        mean / std, and with a reward scale rewrite column S — all in one launch.  Not idempotent."""
        t = _as_rows(store_or_rows)
        S = self.obs_dim
        if t.shape[1] < 2 * S + 1:
            raise ValueError(f"rows of {t.shape[1]} columns have no [s | r | s'] of obs_dim {S}")
        self._on(t, "rows")
        shift, div, mul = self._params()
        spans = [(0, S, 0, 0), (S + 1, S, 0, 0)]
        if self.reward_div is not None:
            spans.append((S, 1, S, 1))
        affine_cols_device(t, spans, shift, div, mul)
        return store_or_rows

    def numpy(self):
        """(mean, std) as host fp32 arrays — what the evaluators subtract and divide by."""
        return self.mean.cpu().numpy(), self.std.cpu().numpy()

    def state_dict(self):
        return {"mean": self.mean.detach().clone(), "std": self.std.detach().clone(), "reward_div": self.reward_div,
                "reward_mul": self.reward_mul}

    def load_state_dict(self, sd):
        other = Normalizer(sd["mean"], sd["std"], sd.get("reward_div"), sd.get("reward_mul"))
        dev = self.mean.device
        self.mean, self.std = other.mean.to(dev), other.std.to(dev)
        self.reward_div, self.reward_mul = other.reward_div, other.reward_mul
        self._packed = None
        return self


def normalize_dataset(replay, max_episode_steps=None, eps=1e-3, stats_from=None):
    """Statistics of the observation columns of `stats_from` (default: `replay` itself), `return_range` of the raw
    rewards when `max_episode_steps` is given, then `Normalizer.apply_` on `replay`; sets `replay.normalizer` and
    returns it.  A store that already has a normalizer raises ValueError: the in-place pass is not idempotent.  Nothing
    else is invalidated (an episode table depends on the done column only).

        train, held = holdout_region(replay, env)
        norm = normalize_dataset(train, T)
        norm.apply_(held)                         # the held-out rows, scaled by the training part's statistics
    """
    if getattr(replay, "normalizer", None) is not None:
        raise ValueError("normalize_dataset: the store already has a normalizer (the in-place pass is not idempotent)")
    src = replay if stats_from is None else stats_from
    t = _as_rows(replay)
    S = getattr(src, "obs_dim", None)
    if S is None:
        S = getattr(replay, "obs_dim", None)
    if S is None:
        raise ValueError("normalize_dataset: neither store carries obs_dim")
    norm = Normalizer.from_stats(column_stats(src, (0, S)), eps=eps, device=t.device)
    if max_episode_steps is not None:
        from .episodes import return_range
        lo, hi = return_range(replay, max_episode_steps)
        norm.with_reward_scale(lo, hi, max_episode_steps)
    norm.apply_(replay)
    replay.normalizer = norm
    return norm
