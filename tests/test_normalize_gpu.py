"""Dataset normalisation on the device (csrc/colstats.hpp through porl_amd/dataloader/normalize.py): the statistics
against the fsum oracle inside the derived bounds of tests/helpers/normalize_cases.py, the affine pass bit for bit against
the fp32 numpy restatement, at every size at which a tile, sweep or lane path changes; then `normalize_dataset`, its
composition with the hold-out, and training on what it wrote."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import normalize_cases as NC
from porl_amd.buffer.replay_buffer import PackedReplay
from porl_amd.dataloader import (DeviceDataset, Normalizer, column_stats, holdout_region, normalize_dataset)
from porl_amd.dataloader.normalize import tile_constants
import porl_amd.ops  # noqa: F401  (registers torch.ops.porl_hip)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VIEWS = ("dense", "row_strided", "offset_base")
# (width, (col0, n_cols)): one column, an odd block, the observation / next-observation spans of a 124-float row, a whole
# number of waves, one past it at an odd base, and the 362 floats of a 734-float row
SPANS = ((3, (0, 1)), (5, (1, 3)), (124, (0, 60)), (124, (61, 60)), (64, (0, 64)), (70, (3, 65)), (734, (0, 362)))


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def _sizes(width):
    T, P = tile_constants()
    if width == 734:
        return (1, 2, 63, 64, 65, T - 1, T, T + 1)
    return (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3) + ((T * P + 1,) if width <= 5 else ())


def _view(host, shape):
    """The device view of the (n, W) host rows: dense; `row_strided`, W of W + 36 columns at a 16-byte aligned base (124
    of 160 for the 124-float row); `offset_base`, the base moved by one float, which forces the 4-byte path."""
    n, w = host.shape
    pad, at = {"dense": (0, 0), "row_strided": (36, 16), "offset_base": (4, 1)}[shape]
    wide = torch.from_numpy(np.random.default_rng(w).integers(-2 ** 31, 2 ** 31, size=(n, w + pad), dtype=np.int64).astype(np.int32))
    wide = wide.view(torch.float32).to(DEV)
    v = wide[:, at:at + w]
    v.copy_(torch.from_numpy(host))
    return v


def _check_stats(st, host, span, names, tag):
    n = host.shape[0]
    col0, c = span
    assert st.n == n and st.mean.shape == st.m2.shape == st.min.shape == st.max.shape == (c,) and st.mean.dtype == np.float64
    for j, case in enumerate(names):                               # no case is left out of any comparison
        x = host[:, col0 + j]
        mean, m2, lo, hi = NC.oracle(x)
        got = (st.mean[j], st.m2[j], st.min[j], st.max[j])
        if np.isnan(x).any():
            assert np.isnan(got).all(), (tag, j, case, got)
        elif np.isinf(x).any():
            assert not np.isfinite(got[0]) and not np.isfinite(got[1]) and got[2] == lo and got[3] == hi, (tag, j, case, got)
        else:
            bm, bv = NC.bounds(x)
            dm, dv = abs(got[0] - mean), abs(got[1] / n - m2 / n)
            assert dm <= bm, (tag, j, case, dm, bm)
            assert dv <= bv, (tag, j, case, dv, bv)
            assert got[2] == lo and got[3] == hi, (tag, j, case)
            if case == "const":
                assert got[1] == 0.0 and got[0] == float(np.float32(0.3)), (tag, j, got)


@pytest.mark.parametrize("width,span", SPANS, ids=[f"w{w}_c{s[0]}_{s[1]}" for w, s in SPANS])
def test_column_stats_against_the_oracle(width, span):
    worst = [0.0, 0.0]
    for n in _sizes(width):
        host, names = NC.interleaved(n, width, span, seed=n + width)
        first = None
        for shape in VIEWS:
            v = _view(host, shape)
            before = _bits(v)
            st = column_stats(v, span)
            again = column_stats(v, span)
            got = np.stack([st.mean, st.m2, st.min, st.max])
            np.testing.assert_array_equal(_bits(got), _bits(np.stack([again.mean, again.m2, again.min, again.max])))   # repeat call
            np.testing.assert_array_equal(_bits(v), before)         # the input is bit-unchanged
            _check_stats(st, host, span, names, (n, shape))
            if first is None:
                first = got
            else:                                                   # dense, strided and the 4-byte path: equal bits
                np.testing.assert_array_equal(_bits(got), _bits(first), err_msg=f"{n} {shape}")
        for j, case in enumerate(names):
            if case in NC.FINITE and case != "const" and n > 1:
                x = host[:, span[0] + j]
                mean, m2, _, _ = NC.oracle(x)
                bm, bv = NC.bounds(x)
                if bm > 0:
                    worst[0] = max(worst[0], abs(first[0, j] - mean) / bm)
                if bv > 0:
                    worst[1] = max(worst[1], abs(first[1, j] / n - m2 / n) / bv)
    print(f"w{width} {span}: worst fraction of the mean bound {worst[0]:.2e}, of the variance bound {worst[1]:.2e}")


# wider than the 1024 columns one block takes: one column into a second chunk (4-byte lanes: the pitch is odd), and a span
# of 16-byte lanes over three chunks, the last one short
CHUNKED = ((1025, (0, 1025)), (2052, (0, 2052)))


@pytest.mark.parametrize("width,span", CHUNKED, ids=[f"w{w}_c{s[0]}_{s[1]}" for w, s in CHUNKED])
def test_column_stats_beyond_one_column_chunk(width, span):
    T, _ = tile_constants()
    for n in (3, T + 1):
        host, names = NC.interleaved(n, width, span, seed=n + width)
        st = column_stats(_view(host, "dense"), span)
        _check_stats(st, host, span, names, (n, "dense"))
        first = np.stack([st.mean, st.m2, st.min, st.max])
        for shape in VIEWS[1:]:                                     # the other pitch and the other lane path: equal bits
            v = _view(host, shape)
            before = _bits(v)
            o = column_stats(v, span)
            np.testing.assert_array_equal(_bits(np.stack([o.mean, o.m2, o.min, o.max])), _bits(first), err_msg=f"{n} {shape}")
            np.testing.assert_array_equal(_bits(v), before)


def test_column_stats_defaults_and_stores():
    S, A, n = 17, 2, 300
    rows = NC.packed_rows(n, S, A, seed=1)
    replay = PackedReplay(rows, S, A, DEV)
    a = column_stats(replay)                                        # (0, obs_dim) of a store that carries obs_dim
    b = column_stats(replay.rows, (0, S))
    c = column_stats(DeviceDataset.from_tensor(replay.rows), (0, S))
    whole = column_stats(replay.rows)                               # every column of a bare tensor
    assert a.mean.shape == (S,) and whole.mean.shape == (2 * S + 2 + A,) and a.device == DEV
    for other in (b, c):
        np.testing.assert_array_equal(_bits(a.m2), _bits(other.m2))
    np.testing.assert_allclose(whole.mean[:S], a.mean, rtol=0, atol=1e-14)   # another n_cols, another order: not the same bits
    np.testing.assert_array_equal(whole.min[:S], a.min)
    parts = [column_stats(replay.rows[lo:hi], (0, S)) for lo, hi in ((0, 100), (100, 101), (101, n))]
    merged = parts[0].merge(*parts[1:])
    assert merged.n == n
    np.testing.assert_allclose(merged.mean, a.mean, rtol=0, atol=1e-14)
    np.testing.assert_allclose(merged.var, a.var, rtol=1e-13)
    np.testing.assert_array_equal(merged.min, a.min)
    out = torch.ops.porl_hip.col_stats(replay.rows, 0, S)
    assert out.shape == (4, S) and out.dtype == torch.float64
    np.testing.assert_array_equal(_bits(out[1]), _bits(a.m2))
    with pytest.raises(ValueError, match="cols"):
        column_stats(replay.rows, (30, 10))
    with pytest.raises(ValueError, match="unit column stride"):
        column_stats(replay.rows[:, ::2])
    with pytest.raises(TypeError, match="float32"):
        column_stats(replay.rows.double())


# ---- the affine pass -----------------------------------------------------------------------------------------------------
def _affine_case(n, S, A, seed):
    """rows of random BIT patterns (NaN payloads, denormals) with finite normal-range values in the s, r, s' and last
    columns; parameters whose divisors are no powers of two."""
    rng = np.random.default_rng(seed)
    W = 2 * S + 2 + A
    rows = rng.integers(-2 ** 31, 2 ** 31, size=(n, W), dtype=np.int64).astype(np.int32).view(np.float32)
    rows[:, :2 * S + 1] = rng.uniform(-3, 3, size=(n, 2 * S + 1)).astype(np.float32)
    rows[:, W - 1] = rng.uniform(-3, 3, size=n).astype(np.float32)
    shift = rng.standard_normal(S + 1).astype(np.float32)
    div = rng.uniform(0.6, 2.9, size=S + 1).astype(np.float32)
    mul = rng.uniform(100, 1000, size=S + 1).astype(np.float32)
    sets = {"s": [(0, S, 0, 0)], "s_s2": [(0, S, 0, 0), (S + 1, S, 0, 0)],
            "s_s2_r": [(0, S, 0, 0), (S + 1, S, 0, 0), (S, 1, S, 1)], "last": [(W - 1, 1, 2, 1)],
            "s_mul": [(0, S, 0, 1)]}                                # S % 4 == 0: 16-byte lanes with the multiply flag
    return rows, shift, div, mul, sets


@pytest.mark.parametrize("shape", VIEWS)
@pytest.mark.parametrize("S", (60, 4))
def test_affine_cols_bit_exact(S, shape):
    A = 2
    T, P = tile_constants()
    for n in (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3) + ((T * P + 1,) if S == 4 else ()):
        host, shift, div, mul, sets = _affine_case(n, S, A, seed=n + S)
        dsh, ddv, dml = (torch.from_numpy(v).to(DEV) for v in (shift, div, mul))
        for name, spans in sets.items():
            want = NC.affine(host, spans, shift, div, mul)
            flat = [v for s in spans for v in s]
            src = _view(host, shape)
            before = _bits(src)
            dst = _view(np.zeros_like(host), "dense" if shape == "row_strided" else "row_strided")
            dst.copy_(src)
            from porl_amd.dataloader.normalize import affine_cols_device
            affine_cols_device(src, spans, dsh, ddv, dml, out=dst)  # into a second buffer
            np.testing.assert_array_equal(_bits(dst), _bits(want), err_msg=f"{n} {name} out of place")
            np.testing.assert_array_equal(_bits(src), before)
            torch.ops.porl_hip.affine_cols(src, flat, dsh, ddv, dml)        # in place
            np.testing.assert_array_equal(_bits(src), _bits(want), err_msg=f"{n} {name} in place")
            touched = np.zeros(host.shape[1], dtype=bool)
            for c0, c, _, _ in spans:
                touched[c0:c0 + c] = True
            np.testing.assert_array_equal(_bits(src)[:, ~touched], _bits(host)[:, ~touched])   # payloads outside the spans


def test_affine_special_values_and_true_division():
    x, d = NC.reciprocal_pairs(128)
    assert x.size >= 100
    C = x.size
    host = np.random.default_rng(0).uniform(1, 2, size=(5, C)).astype(np.float32)
    host[0] = x
    host[1] = np.float32(-0.0)
    host[2] = np.float32(np.nan)
    shift = np.zeros(C, dtype=np.float32)
    want = NC.affine(host, [(0, C, 0, 0)], shift, d)
    recip = (host[0] * (np.float32(1) / d).astype(np.float32)).astype(np.float32)
    assert (_bits(want[0]) != _bits(recip)).all()                    # a reciprocal multiplication would show on every column
    for shape in VIEWS:
        v = _view(host, shape)
        norm = Normalizer(torch.from_numpy(shift).to(DEV), torch.from_numpy(d).to(DEV))
        got = norm.apply(v)
        assert got.shape == v.shape and got.is_contiguous()
        np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))
        np.testing.assert_array_equal(_bits(got[3:]), _bits(want[3:]))
        assert (_bits(got[1]) == _bits(np.float32(-0.0))).all()      # -0.0 - 0.0 = -0.0, / d > 0 = -0.0
        assert torch.isnan(got[2]).all()                             # NaN in, NaN out
        np.testing.assert_array_equal(_bits(v), _bits(host))         # apply does not write its input
        one = norm.apply(v[0])
        assert one.shape == (C,)
        np.testing.assert_array_equal(_bits(one), _bits(want[0]))
    # subtract-then-divide and divide-then-multiply are not contracted: each keeps its own rounding
    rng = np.random.default_rng(1)
    host = rng.uniform(-3, 3, size=(257, 9)).astype(np.float32)
    sh, dv, ml = (rng.uniform(0.6, 2.9, size=9).astype(np.float32) for _ in range(3))
    v = _view(host, "dense")
    torch.ops.porl_hip.affine_cols(v, [0, 9, 0, 1], *(torch.from_numpy(a).to(DEV) for a in (sh, dv, ml)))
    np.testing.assert_array_equal(_bits(v), _bits(NC.affine(host, [(0, 9, 0, 1)], sh, dv, ml)))


def test_affine_out_is_checked():
    from porl_amd.dataloader.normalize import affine_cols_device
    rng = np.random.default_rng(3)
    host = rng.uniform(-3, 3, size=(40, 24)).astype(np.float32)
    sh, dv = (torch.from_numpy(rng.uniform(0.6, 2.9, size=8).astype(np.float32)).to(DEV) for _ in range(2))
    wide = torch.from_numpy(host).to(DEV)
    src, spans = wide[:, :8], [(0, 8, 0, 0)]
    with pytest.raises(TypeError, match="out.*float32"):
        affine_cols_device(src, spans, sh, dv, out=torch.empty(40, 8, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="out.*unit column stride"):
        affine_cols_device(src, spans, sh, dv, out=wide[:, 8::2])
    with pytest.raises(ValueError, match=r"out: expected \(40, >= 8\)"):
        affine_cols_device(src, spans, sh, dv, out=torch.empty(39, 8, device=DEV))
    for bad in (wide[:, 4:12], wide.view(-1)[:40 * 8].view(40, 8)):  # shifted by half a block; the same memory at another pitch
        with pytest.raises(ValueError, match="out: partly overlaps"):
            affine_cols_device(src, spans, sh, dv, out=bad)
    np.testing.assert_array_equal(_bits(wide), _bits(host))          # nothing was launched
    affine_cols_device(src, spans, sh, dv, out=wide[:, 16:24])       # another column block of the same rows is no overlap
    want = NC.affine(host, spans, sh.cpu().numpy(), dv.cpu().numpy())[:, :8]
    np.testing.assert_array_equal(_bits(wide[:, 16:24]), _bits(want))
    np.testing.assert_array_equal(_bits(wide[:, :16]), _bits(host[:, :16]))


# ---- normalize_dataset -------------------------------------------------------------------------------------------------
S17, A2 = 17, 2


def _store_rows():
    T, _ = tile_constants()
    return NC.packed_rows(2 * T + 3, S17, A2, seed=7)


def test_normalize_dataset_matches_the_restatement():
    rows = _store_rows()
    steps = 30
    want, mean32, std32, rdiv, rmul = NC.normalize_rows(rows, S17, max_episode_steps=steps)
    replay = PackedReplay(rows, S17, A2, DEV)
    norm = normalize_dataset(replay, steps)
    assert replay.normalizer is norm and norm.obs_dim == S17
    np.testing.assert_array_equal(_bits(norm.mean), _bits(mean32))
    np.testing.assert_array_equal(_bits(norm.std), _bits(std32))
    assert (norm.reward_div, norm.reward_mul) == (float(rdiv), float(rmul))
    np.testing.assert_array_equal(_bits(replay.rows), _bits(want))
    np.testing.assert_array_equal(_bits(replay.rows[:, 2 * S17 + 1:]), _bits(rows[:, 2 * S17 + 1:]))    # d, a untouched
    with pytest.raises(ValueError, match="already has a normalizer"):
        normalize_dataset(replay, steps)
    np.testing.assert_array_equal(_bits(replay.rows), _bits(want))
    # Every element is y = fl(fl(x - m32) / s32) with |y| < 2: two roundings, each relative 2^-24, so |y - y_exact| <
    # 2 * 2^-24 * 2 = 2.4e-7, and the column mean of y differs from (mean64 - m32) / s32 — itself below 2^-24 |mean| / s32 <
    # 1e-8 for U(-3, 3) — by less than that even if every rounding went the same way: 1e-6 holds with a factor 4 to
    # spare.  std(y) = std / (std + eps) = 1 - eps / std + O(eps^2) = 1 - 1e-3 / 1.73 = 1 - 5.8e-4 (eps shifts it), the
    # roundings add at most 2.4e-7 relative: 2e-3 holds with a factor 3 to spare.
    after = column_stats(replay)
    print(f"after: max |mean| = {np.abs(after.mean).max():.3e}, max |std - 1| = {np.abs(after.std - 1).max():.3e}")
    assert np.abs(after.mean).max() <= 1e-6
    assert np.abs(after.std - 1).max() <= 2e-3
    plain = PackedReplay(rows, S17, A2, DEV)                        # without a reward scale the reward column is untouched
    n2 = normalize_dataset(plain)
    assert n2.reward_div is None
    np.testing.assert_array_equal(_bits(plain.rows), _bits(NC.normalize_rows(rows, S17)[0]))
    np.testing.assert_array_equal(_bits(plain.rows[:, S17]), _bits(rows[:, S17]))


def test_composition_with_the_holdout():
    rows = _store_rows()
    replay = PackedReplay(rows, S17, A2, DEV, seed=3)
    xr, yr = (-3.0, 0.5), (-1.0, 3.0)
    train, held = holdout_region(replay, x_range=xr, y_range=yr)
    m = (rows[:, 0] >= xr[0]) & (rows[:, 0] <= xr[1]) & (rows[:, 1] >= yr[0]) & (rows[:, 1] <= yr[1])
    assert 0 < m.sum() < len(rows) and len(held) == m.sum()
    steps = 25
    norm = normalize_dataset(train, steps)
    norm.apply_(held)
    want_train, mean32, std32, rdiv, rmul = NC.normalize_rows(rows[~m], S17, max_episode_steps=steps)
    np.testing.assert_array_equal(_bits(train.rows), _bits(want_train))
    spans = [(0, S17, 0, 0), (S17 + 1, S17, 0, 0), (S17, 1, S17, 1)]
    want_held = NC.affine(rows[m], spans, np.append(mean32, np.float32(0)), np.append(std32, rdiv),
                          np.append(np.ones(S17, np.float32), rmul))
    np.testing.assert_array_equal(_bits(held.rows), _bits(want_held))             # the train statistics, not its own
    own = NC.normalize_rows(rows[m], S17)[1]
    assert not np.array_equal(own, mean32)
    assert train.normalizer is norm and getattr(held, "normalizer", None) is None
    np.testing.assert_array_equal(_bits(replay.rows), _bits(rows))                # the source store keeps its raw rows


def _make_por(S, H, B, seed=0):
    from porl_amd.agent.por import POR
    torch.manual_seed(seed)
    args = SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=2, layer_norm=False, feature_dim=256, action_size=A2, max_batch=B)
    return POR(args, 1000, 0.9, 10.0, device=DEV)


def test_training_reads_what_was_written():
    rows = _store_rows()
    H, B, steps = 64, 32, 30
    dev_store = PackedReplay(rows, S17, A2, DEV, seed=1)
    normalize_dataset(dev_store, steps)
    host_store = PackedReplay(NC.normalize_rows(rows, S17, max_episode_steps=steps)[0], S17, A2, DEV, seed=1)
    assert torch.equal(dev_store.rows.view(torch.int32), host_store.rows.view(torch.int32))
    x, y = _make_por(S17, H, B), _make_por(S17, H, B)
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        idx = torch.randperm(len(rows), generator=g)[:B].to(DEV)
        lx = x.update_from_replay(dev_store, B, indices=idx)
        ly = y.update_from_replay(host_store, B, indices=idx)
        assert lx == ly and all(np.isfinite(v) for v in np.ravel(lx)), (lx, ly)
    for e in (x, y):
        if hasattr(e, "flush"):
            e.flush()
    sx, sy = x.state_dict(), y.state_dict()
    assert sx.keys() == sy.keys()
    for k in sx:
        assert torch.equal(sx[k], sy[k]), k
