"""The A* labelling pass on the device (porl_amd/dataloader/astar.py over csrc/astar.hpp) against the reference's
recorded results (tests/golden/astar_rows.npz) and against the numpy restatement (tests/helpers/astar_cases.py).
Every comparison is exact: statuses, path lengths, and the float32 values bit for bit.  The rows of the fixture and of
the generator keep every comparison of the pass away from a tie (astar_cases.margins_ok), so two correct fp64
implementations cannot differ.  No row here may report status 7 (sweep bound reached)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import astar_cases as AC
from porl_amd import _native as N
from porl_amd import ops as O  # noqa: F401  (registers torch.ops.porl_hip)
from porl_amd.dataloader import DeviceDataset, EpochLoader, astar_values, label_dataset, label_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_ROWS = 96               # more workgroups than one per CU of an XCD (32), and not a power of two


def run(rows, **kw):
    """astar_values on numpy or device rows -> numpy (status, path_len, value); never status 7."""
    t = torch.from_numpy(rows).to(DEV) if isinstance(rows, np.ndarray) else rows
    value, path_len, status = astar_values(t, **kw)
    assert value.dtype == torch.float32 and path_len.dtype == torch.int32 and status.dtype == torch.int32
    assert value.shape == path_len.shape == status.shape == (t.shape[0],)
    status = status.cpu().numpy()
    assert (status != AC.NOT_CONVERGED).all()
    return status, path_len.cpu().numpy(), value.cpu().numpy()


def same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


@pytest.fixture(scope="module")
def cases():
    rows = AC.make_rows(N_ROWS, seed=1)
    return rows, AC.label_all(rows)


def test_golden_rows_match_the_reference():
    z, _ = load_golden("astar_rows")
    rows, kept = z["rows"], z["kept"]
    status, path_len, value = run(rows)
    np.testing.assert_array_equal(status == 0, kept)
    np.testing.assert_array_equal(path_len[kept], z["path_len"][kept])
    assert (path_len[~kept] == 0).all()
    np.testing.assert_array_equal(value.view(np.uint32), z["value"].view(np.uint32))
    rec = label_rows(torch.from_numpy(rows).to(DEV))
    assert rec.shape == (int(kept.sum()), 361) and rec.dtype == torch.float32
    want = np.concatenate([rows[kept, :360], z["value"][kept, None]], axis=1)
    np.testing.assert_array_equal(rec.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_generated_rows_match_the_restatement(cases):
    rows, want = cases
    assert set(want[0].tolist()) == {0, 1, 2, 3, 4, 5} and want[1].max() > 100
    same(run(rows), want)
    for i in (0, 9, 57):                                          # one workgroup
        same(run(rows[i:i + 1]), tuple(w[i:i + 1] for w in want))
    wide = torch.full((N_ROWS, 1001), float("nan"), device=DEV)    # the rows as a view into a wider buffer
    wide[:, 7:741] = torch.from_numpy(rows).to(DEV)
    view = wide[:, 7:741]
    assert not view.is_contiguous()
    same(run(view), want)
    same(run(wide[::2, 7:741]), tuple(w[::2] for w in want))
    perm = np.random.default_rng(0).permutation(N_ROWS)
    same(run(rows[perm]), tuple(w[perm] for w in want))


def test_empty_field_closed_form():
    inside = [(-100, 0), (99, 0), (0, -50), (0, 49), (-100, -50), (99, 49), (-100, 49), (99, -50), (37, -12), (-5, 44),
              (1, 0), (0, 1), (-1, -1), (60, 0)]
    beyond = [(-101, 0), (100, 0), (0, -51), (0, 50), (-101, -51), (100, 50)]
    rows = np.stack([AC.empty_field_row(dx, dy) for dx, dy in inside + beyond])
    status, path_len, value = run(rows)
    k = len(inside)
    np.testing.assert_array_equal(status[:k], 0)
    np.testing.assert_array_equal(path_len[:k], [max(abs(dx), abs(dy)) + 1 for dx, dy in inside])
    np.testing.assert_array_equal(value[:k].view(np.uint32),
                                  np.array([AC.value_of(n) for n in path_len[:k]], dtype=np.float32).view(np.uint32))
    np.testing.assert_array_equal(status[k:], AC.GOAL_OFF_GRID)
    np.testing.assert_array_equal(path_len[k:], 0)
    np.testing.assert_array_equal(value[k:], 0.0)


@pytest.mark.parametrize("grid", [dict(resolution=0.2), dict(resolution=0.05, min_x=-5.0, max_x=5.0, min_y=-2.5, max_y=2.5)],
                         ids=["100x50", "200x100_at_0.05"])
def test_other_grids_match_the_restatement(grid):
    p = AC.params(**grid)
    assert AC.grid_dims(p) in ((100, 50), (200, 100))
    rows = AC.make_rows(36, seed=2, p=p)
    want = AC.label_all(rows, p)
    assert (want[0] == 0).sum() >= 8 and len(set(want[0].tolist())) >= 4
    same(run(rows, **grid), want)


def test_every_status_but_not_converged():
    made = {AC.TOO_CLOSE: AC.make_row("too_close", 7), AC.GOAL_IS_START: AC.make_row("start", 7),
            AC.GOAL_OFF_GRID: AC.make_row("off_grid", 7), AC.GOAL_BLOCKED: AC.make_row("on_return", 7),
            AC.UNREACHABLE: AC.make_row("sealed_out", 7), AC.OK: AC.make_row("pillar", 7)}
    for what, col in (("nan goal", 363), ("inf goal", 364), ("nan heading", 362), ("nan pose", 360)):
        r = AC.make_row("pillar", 8)
        r[col] = np.inf if what.startswith("inf") else np.nan
        made[what] = r
    # numpy's min: one NaN beam hides a beam that is too close; an infinite beam is just "no return"
    hidden = AC.make_row("too_close", 9)
    hidden[int(np.argmax(hidden[:360]))] = np.nan
    far = AC.make_row("pillar", 9)
    far[:360][far[:360] >= AC.NO_RETURN] = np.inf
    keys = list(made)
    rows = np.stack([made[k] for k in keys] + [hidden, far])
    status, path_len, value = run(rows)
    for k, s in zip(keys, status):
        assert s == (k if isinstance(k, int) else AC.NON_FINITE), (k, s)
    assert set(status.tolist()) >= {0, 1, 2, 3, 4, 5, 6}
    same((status, path_len, value), AC.label_all(rows))
    assert status[-2] != AC.TOO_CLOSE and status[-1] == AC.OK
    assert ((status == 0) == (path_len > 0)).all() and ((status == 0) == (value > 0)).all()


def test_bad_arguments_raise():
    rows = torch.zeros(4, 734, device=DEV)
    with pytest.raises(N.NativeError, match="resolution"):
        astar_values(rows, resolution=0.01)
    with pytest.raises(N.NativeError, match="resolution"):
        astar_values(rows, resolution=0.0)
    with pytest.raises(ValueError):
        astar_values(rows[:, :364])
    with pytest.raises(ValueError):
        astar_values(rows.t().contiguous().t())
    with pytest.raises(ValueError):
        astar_values(rows.double())
    v, l, s = astar_values(rows[:0])
    assert v.shape == l.shape == s.shape == (0,)
    assert label_rows(rows[:0]).shape == (0, 361)


def test_loader_path(cases):
    rows, want = cases
    kept = want[0] == 0
    records = np.concatenate([rows[kept, :360], want[2][kept, None]], axis=1)
    src = DeviceDataset(rows, DEV)
    ds = label_dataset(src, chunk_rows=40)                        # three chunks, the last one short
    assert isinstance(ds, DeviceDataset) and ds.width == 361 and len(ds) == int(kept.sum())
    np.testing.assert_array_equal(ds.rows.cpu().numpy().view(np.uint32), records.view(np.uint32))
    loader = EpochLoader(ds, 7, shuffle=True)
    order = lambda a: a[np.lexsort(a.T[::-1])]
    epochs = []
    for _ in range(2):
        batches = [b.cpu().numpy() for b in loader]
        assert len(batches) == len(loader) and all(b.shape[1] == 361 for b in batches)
        assert [b.shape[0] for b in batches] == [7] * (len(ds) // 7) + ([len(ds) % 7] if len(ds) % 7 else [])
        got = np.concatenate(batches)
        np.testing.assert_array_equal(order(got), order(records))   # every labelled row exactly once
        epochs.append(got)
    assert not np.array_equal(epochs[0], epochs[1])


def test_operator_agrees(cases):
    rows, want = cases
    t = torch.from_numpy(rows).to(DEV)
    v, l, s = torch.ops.porl_hip.astar_label(t)
    same((s.cpu().numpy(), l.cpu().numpy(), v.cpu().numpy()), want)
    v2, l2, s2, sweeps = astar_values(t, return_sweeps=True)
    assert torch.equal(v, v2) and torch.equal(l, l2) and torch.equal(s, s2)
    sweeps = sweeps.cpu().numpy()
    searched = np.isin(want[0], (AC.OK, AC.UNREACHABLE))
    assert (sweeps[~searched] == 0).all() and (sweeps[searched] >= 1).all() and (sweeps < 20000).all()
    p = AC.params(resolution=0.2)
    rows2 = AC.make_rows(12, seed=3, p=p)
    v, l, s = torch.ops.porl_hip.astar_label(torch.from_numpy(rows2).to(DEV), resolution=0.2)
    same((s.cpu().numpy(), l.cpu().numpy(), v.cpu().numpy()), AC.label_all(rows2, p))
