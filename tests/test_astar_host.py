"""The A* labelling pass without a GPU: the numpy restatement (tests/helpers/astar_cases.py) against the reference's
recorded results (tests/golden/astar_rows.npz, written by tests/helpers/gen_astar_golden.py), the C ABI's declaration,
and the argument checks of porl_astar_label, which all come before its first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from helpers import astar_cases as AC
from porl_amd import _native as N
from porl_amd import ops as O  # noqa: F401  (registers torch.ops.porl_hip)


def test_restatement_reproduces_the_reference():
    z, _ = load_golden("astar_rows")
    rows = z["rows"]
    assert rows.dtype == np.float32 and rows.shape[1] == 734 and rows.shape[0] >= 35
    status, path_len, value = AC.label_all(rows)
    np.testing.assert_array_equal(status == 0, z["kept"])
    np.testing.assert_array_equal(path_len[z["kept"]], z["path_len"][z["kept"]])
    assert (z["path_len"][~z["kept"]] <= 1).all()                  # a dropped row: the filter (0) or a one-node path
    np.testing.assert_array_equal(value.view(np.uint32), z["value"].view(np.uint32))
    for r in rows:
        assert AC.margins_ok(r)


def test_fixture_covers_the_situations():
    z, _ = load_golden("astar_rows")
    status, path_len, _ = AC.label_all(z["rows"])
    assert set(status.tolist()) == {0, 1, 2, 3, 4, 5}
    assert path_len.max() > 100                                     # the detour round the U-shaped room
    heading = z["rows"][:, 362]
    assert (np.abs(np.abs(heading) - np.pi) < 0.03).sum() >= 2      # near +pi and near -pi
    assert (heading > 3.1).any() and (heading < -3.1).any()
    empty = [i for i, r in enumerate(z["rows"]) if not ((r[:360] > 0.15) & (r[:360] < 3.5)).any()]
    assert any(z["kept"][i] for i in empty)                         # a labelled row with an empty map


def test_restatement_on_hand_made_maps():
    occ = np.zeros((7, 5), dtype=bool)
    assert AC.shortest_pair(occ, (0, 0), (6, 4)) == (2, 4)
    occ[3, :4] = True                                               # a wall with its gap at the top
    assert AC.shortest_pair(occ, (0, 0), (6, 0)) == (2, 6)          # up to the gap and down again
    occ[3, 4] = True
    assert AC.shortest_pair(occ, (0, 0), (6, 0)) is None
    assert AC.shortest_pair(occ, (3, 0), (0, 0)) == (3, 0)          # a blocked start still expands


def test_abi_declares_the_entry_point():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    assert re.search(r"\bint\s+porl_astar_label\s*\(", txt)
    assert "porl_astar_label" in N.SYMBOLS
    assert N.ABI_VERSION == 12 and N.lib().porl_abi_version() == 12
    for k, name in enumerate(("LABELLED", "TOO_CLOSE", "GOAL_IS_START", "GOAL_OFF_GRID", "GOAL_BLOCKED", "UNREACHABLE",
                              "NON_FINITE", "NOT_CONVERGED")):
        assert re.search(rf"PORL_ASTAR_{name}\s*=\s*{k}\b", txt), name


def _call(**over):
    """porl_astar_label on host buffers; every case below is rejected before anything is launched."""
    lib = N.lib()
    n = 4
    a = dict(rows=(C.c_float * (n * 734))(), stride=734, n_rows=n, params=N.AstarParams(0.1, 0.13, -10., 10., -5., 5., 0.15, 3.5,
                                                                                     360, 360, 362, 363),
             dirs=(C.c_double * 720)(), table=(C.c_float * 20002)(), n_values=20002, value=(C.c_float * n)(),
             path_len=(C.c_int32 * n)(), status=(C.c_int32 * n)(), sweeps=None)
    a.update(over)
    rc = lib.porl_astar_label(a["rows"], a["stride"], a["n_rows"], a["params"] and C.byref(a["params"]), a["dirs"], a["table"],
                              a["n_values"], a["value"], a["path_len"], a["status"], a["sweeps"], None)
    return rc, lib.porl_last_error().decode()


@pytest.mark.parametrize("arg", ["rows", "params", "dirs", "table", "value", "path_len", "status"])
def test_null_pointers_are_rejected_by_name(arg):
    rc, msg = _call(**{arg: None})
    name = {"dirs": "beam_dirs", "table": "value_table"}.get(arg, arg)
    assert rc == -1 and f"null {name}" in msg, (rc, msg)


def test_bad_sizes_are_rejected_by_name():
    for n in (0, -1, 1 << 31):
        rc, msg = _call(n_rows=n)
        assert rc == -1 and "n_rows" in msg, (rc, msg)
    for stride in (0, 364):                                        # the goal's y is column 364: 365 floats are read
        rc, msg = _call(stride=stride)
        assert rc == -1 and "row_stride" in msg, (rc, msg)
    rc, msg = _call(n_values=20001)
    assert rc == -1 and "n_values" in msg and "value_table" in msg, (rc, msg)


def test_bad_grids_are_rejected_by_name():
    P = N.AstarParams
    rc, msg = _call(params=P(0.01, 0.13, -10., 10., -5., 5., 0.15, 3.5, 360, 360, 362, 363))     # 2000 x 1000 cells
    assert rc == -1 and "resolution" in msg and "2000 x 1000" in msg, (rc, msg)
    rc, msg = _call(params=P(0.07, 0.13, -10., 10., -5., 5., 0.15, 3.5, 360, 360, 362, 363))     # 286 x 143: 160 KB of pairs
    assert rc == -1 and "resolution" in msg, (rc, msg)
    for bad in (0.0, -0.1, float("nan")):
        rc, msg = _call(params=P(bad, 0.13, -10., 10., -5., 5., 0.15, 3.5, 360, 360, 362, 363))
        assert rc == -1 and ("resolution" in msg or "finite" in msg), (rc, msg)
    rc, msg = _call(params=P(0.1, 0.13, 10., -10., -5., 5., 0.15, 3.5, 360, 360, 362, 363))
    assert rc == -1 and "min_x" in msg, (rc, msg)
    rc, msg = _call(params=P(0.1, 0.13, 1., 10., -5., 5., 0.15, 3.5, 360, 360, 362, 363))         # the robot is not in the window
    assert rc == -1 and "robot" in msg, (rc, msg)
    rc, msg = _call(params=P(0.1, 0.13, -10., 10., -5., 5., 0.15, 3.5, 0, 360, 362, 363))
    assert rc == -1 and "n_beams" in msg, (rc, msg)
    rc, msg = _call(params=P(0.1, 0.13, -10., 10., -5., 5., 0.15, 3.5, 360, 360, 362, -1))
    assert rc == -1 and "offset" in msg, (rc, msg)


def test_python_entry_points_have_no_cpu_path():
    import torch
    from porl_amd.dataloader import DeviceDataset, astar_values, label_dataset, label_rows      # noqa: F401
    rows = torch.zeros(3, 734)
    with pytest.raises(N.NativeError):
        astar_values(rows)
    with pytest.raises(N.NativeError):
        label_rows(rows)
    with pytest.raises(N.NativeError):
        torch.ops.porl_hip.astar_label(rows)
    with pytest.raises(N.NativeError):
        DeviceDataset.from_tensor(rows)
    with pytest.raises(TypeError):
        astar_values(rows, resolutoin=0.1)
