"""The hold-out partition on the device (csrc/partition.hpp through porl_amd/dataloader/holdout.py) against the
reference's recorded results (tests/golden/holdout_ref.npz) and against numpy's `rows[~m]` / `rows[m]` on the host, at
every size at which a tile, sweep or lane path changes."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import holdout_cases as HC
from porl_amd.buffer.replay_buffer import PackedReplay
from porl_amd.dataloader import (DeviceDataset, EpochLoader, generate_test_generlaization_data, holdout_region,
                                 partition_rows)
from porl_amd.dataloader.holdout import tile_constants
from porl_amd.util import util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("observations", "actions", "rewards", "terminals")
SHAPES = ("w9", "w124", "w126", "row_strided", "offset_base", "int64_vec", "fp32_vec")


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def _sizes():
    T, P = tile_constants()
    return (1, 2, 63, 64, 65, T - 1, T, T + 1, T * P + 1)


def _payload(n, w, seed):
    """fp32 rows of random BIT patterns (NaN payloads, -0.0, denormals included): the copy must keep every one."""
    bits = np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, size=(n, w), dtype=np.int64).astype(np.int32)
    return torch.from_numpy(bits).to(DEV).view(torch.float32)


def _view(shape, n):
    """-> the device view to partition; the tensor that owns its memory is kept alive by the view."""
    if shape == "w9":
        return _payload(n, 9, 1)                                    # 36-byte rows: no 16-byte path
    if shape == "w124":
        return _payload(n, 124, 2)                                  # 496 bytes, aligned
    if shape == "w126":
        return _payload(n, 126, 3)                                  # 504 bytes: 4-byte lanes
    if shape == "row_strided":
        return _payload(n, 160, 4)[:, 16:140]                       # 124 of 160 columns, 16-byte aligned base and pitch
    if shape == "offset_base":
        return _payload(n, 128, 5)[:, 1:125]                        # base moved by one float
    if shape == "int64_vec":
        return torch.from_numpy(np.random.default_rng(6).integers(-2 ** 62, 2 ** 62, size=n)).to(DEV)
    return _payload(n, 1, 7).view(-1)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", range(9))
def test_partition_matches_numpy(n, shape):
    n = _sizes()[n]
    T, _ = tile_constants()
    x = _view(shape, n)
    before = _bits(x)
    host = before.reshape(n, -1)
    w = host.shape[1]
    for name, m in HC.patterns(n, T).items():
        part = partition_rows(x, torch.from_numpy(m).to(DEV), return_index=True)
        want, n_kept, index = HC.stable_partition(host, m)
        assert part.n_kept == n_kept == int((~m).sum()), name
        assert part.rows.shape == x.shape and part.rows.dtype == x.dtype
        np.testing.assert_array_equal(_bits(part.rows).reshape(-1, w), want, err_msg=name)
        np.testing.assert_array_equal(_bits(part.kept).reshape(-1, w), host[~m], err_msg=name)
        np.testing.assert_array_equal(_bits(part.held).reshape(-1, w), host[m], err_msg=name)
        np.testing.assert_array_equal(part.index.cpu().numpy(), index, err_msg=name)
        np.testing.assert_array_equal(part.index.cpu().numpy(), np.concatenate([np.flatnonzero(~m), np.flatnonzero(m)]))
    np.testing.assert_array_equal(_bits(x), before)                 # the input is never written


def _box_rows(n, w, seed):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(0, 1, size=(n, w)).astype(np.float32)
    lo = np.float32(0.1)
    edge = [lo, np.nextafter(lo, np.float32(-1)), np.nextafter(lo, np.float32(1)), np.float32(0.7),
            np.nextafter(np.float32(0.7), np.float32(1)), np.float32(np.nan), np.float32(-0.0), np.float32(0.0)]
    for k, v in enumerate(edge):
        if 2 * k + 1 < n:
            rows[2 * k, 0], rows[2 * k + 1, 1] = v, v
            rows[2 * k, 1], rows[2 * k + 1, 0] = np.float32(0.3), np.float32(0.3)
    return rows


@pytest.mark.parametrize("n", range(9))
def test_box_form_agrees_with_mask_form_and_numpy(n):
    """Bounds that fp32 cannot represent (0.1, 0.7) compare as numpy's fp32 comparison does; NaN, -0.0 and coordinates
    one ulp either side of an edge included.  Columns other than (0, 1) and a strided view are read in place."""
    n = _sizes()[n]
    for w, cols, xr, yr in ((9, (0, 1), (0.1, 0.7), (0.1, 0.7)), (12, (1, 0), (0.0, 0.3), (0.1, 1.0))):
        host = _box_rows(n, w, n + w)
        wide = torch.from_numpy(np.concatenate([host, host], axis=1)).to(DEV)
        for x in (wide[:, :w].contiguous(), wide[:, w:]):
            m = HC.held_mask(host, xr, yr, cols)
            a = partition_rows(x, x_range=xr, y_range=yr, cols=cols, return_index=True)
            b = partition_rows(x, torch.from_numpy(m).to(DEV), return_index=True)
            assert a.n_kept == b.n_kept == int((~m).sum())
            np.testing.assert_array_equal(_bits(a.rows), _bits(b.rows))
            np.testing.assert_array_equal(a.index.cpu().numpy(), b.index.cpu().numpy())
            np.testing.assert_array_equal(_bits(a.rows), HC.stable_partition(_bits(host), m)[0])


@pytest.mark.parametrize("env", HC.ENV_NAMES)
def test_golden_dict_form(env):
    z, _ = load_golden("holdout_ref")
    for fn in (generate_test_generlaization_data, U.generate_test_generlaization_data):
        ds = {k: torch.from_numpy(z[f"{env}/in/{k}"]).to(DEV) for k in KEYS}
        got = fn(ds, env, 1)                                        # env_idx is accepted and ignored
        assert got is ds                                            # updated in place and returned
        for k in KEYS:
            want = z[f"{env}/out/{k}"]
            assert tuple(got[k].shape) == want.shape and got[k].dtype == torch.float32
            np.testing.assert_array_equal(_bits(got[k]), _bits(want), err_msg=k)


@pytest.mark.parametrize("env", HC.ENV_NAMES)
def test_golden_through_holdout_region(env):
    """The dict dataset packed as [s | r | s' | d | a] rows (S = 4, A = 2): train.rows are the rows the reference keeps,
    held.rows the rows it deletes."""
    z, _ = load_golden("holdout_ref")
    obs, act, rew, term = (z[f"{env}/in/{k}"] for k in KEYS)
    rows = np.concatenate([obs, rew[:, None], np.roll(obs, -1, axis=0), term[:, None], act], axis=1)
    replay = PackedReplay(rows, 4, 2, DEV, seed=5)
    replay.draws = 3
    train, held = holdout_region(replay, env)
    m = HC.held_mask(obs, *HC.box_for(env))
    np.testing.assert_array_equal(_bits(train.rows), _bits(rows[~m]))
    np.testing.assert_array_equal(_bits(held.rows), _bits(rows[m]))
    np.testing.assert_array_equal(_bits(train.rows[:, :4]), _bits(z[f"{env}/out/observations"]))
    np.testing.assert_array_equal(_bits(train.rows[:, 4]), _bits(z[f"{env}/out/rewards"]))
    np.testing.assert_array_equal(_bits(train.rows[:, 10:]), _bits(z[f"{env}/out/actions"]))
    np.testing.assert_array_equal(_bits(replay.rows), _bits(rows))
    for part in (train, held):
        assert (part.obs_dim, part.act_dim, part.draws) == (4, 2, 0) and part.width == 12
    assert len(train) + len(held) == len(replay) and replay.draws == 3
    assert len({train.seed, held.seed, replay.seed}) == 3           # the parts draw streams of their own
    assert train.rows.untyped_storage().data_ptr() == held.rows.untyped_storage().data_ptr()   # one buffer, one copy
    only_train = U.generate_test_generlaization_data(replay, env)
    np.testing.assert_array_equal(_bits(only_train.rows), _bits(rows[~m]))
    i1, i2 = train.sample_indices(16).clone(), held.sample_indices(16).clone()
    assert not torch.equal(i1, i2) and train.draws == held.draws == 1


def test_arguments():
    x = torch.zeros(8, 4, device=DEV)
    m = torch.zeros(8, dtype=torch.uint8, device=DEV)
    for kw in (dict(), dict(held=m, x_range=(0, 1), y_range=(0, 1)), dict(x_range=(0, 1)), dict(held=m, y_range=(0, 1))):
        with pytest.raises(ValueError, match="exactly one"):
            partition_rows(x, **kw)
    with pytest.raises(ValueError, match="cols"):
        partition_rows(x, x_range=(0, 1), y_range=(0, 1), cols=(0, 4))
    with pytest.raises(ValueError, match="held"):
        partition_rows(x, m[:7])
    with pytest.raises(ValueError, match="unit column stride"):
        partition_rows(torch.zeros(8, 8, device=DEV)[:, ::2], m)
    with pytest.raises(TypeError, match="fp32"):
        partition_rows(torch.zeros(8, 4, dtype=torch.int32, device=DEV), x_range=(0, 1), y_range=(0, 1))
    with pytest.raises(TypeError, match="dtype"):
        partition_rows(torch.zeros(8, 4, dtype=torch.float16, device=DEV), m)
    replay = PackedReplay(np.zeros((8, 12), dtype=np.float32), 4, 2, DEV)
    with pytest.raises(ValueError, match="exactly one"):
        holdout_region(replay)
    with pytest.raises(ValueError, match="exactly one"):
        holdout_region(replay, "hopper", x_range=(0, 1), y_range=(0, 1))
    empty = partition_rows(x[:0], m[:0], return_index=True)
    assert empty.n_kept == 0 and empty.rows.shape == (0, 4) and empty.index.numel() == 0
    both = partition_rows(DeviceDataset.from_tensor(x), m.bool())    # a DeviceDataset, a bool mask
    assert both.n_kept == 8 and both.held.shape == (0, 4)
    train, held = holdout_region(replay, x_range=(-1, 1), y_range=(-1, 1))      # everything held: an empty train part
    assert len(train) == 0 and len(held) == 8
