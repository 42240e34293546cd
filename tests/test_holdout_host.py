"""The hold-out partition without a GPU: the numpy restatement (tests/helpers/holdout_cases.py) against the reference's
recorded results (tests/golden/holdout_ref.npz, written by tests/helpers/gen_holdout_golden.py), the C ABI's declaration,
and the argument checks of the new entry points, which all come before their first device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden
from helpers import holdout_cases as HC
from porl_amd import _native as N

ENTRY_POINTS = ("porl_partition_workspace", "porl_partition_mask", "porl_partition_rows")
KEYS = ("observations", "actions", "rewards", "terminals")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)


def _case(z, env):
    return {k: z[f"{env}/in/{k}"] for k in KEYS}, {k: z[f"{env}/out/{k}"] for k in KEYS}


@pytest.mark.parametrize("env", HC.ENV_NAMES)
def test_restatement_reproduces_the_reference(env):
    z, _ = load_golden("holdout_ref")
    ds, want = _case(z, env)
    for k, v in HC.golden_datasets()[env].items():                  # the fixture holds the generator's datasets
        np.testing.assert_array_equal(_bits(v), _bits(ds[k]))
    got = HC.generate_test_generlaization_data(ds, env)
    held = HC.held_mask(ds["observations"], *HC.box_for(env))
    assert 0 < held.sum() < HC.N_ROWS
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]))
        out, n_kept, index = HC.stable_partition(ds[k], held)       # the partition's front IS the reference's result
        assert n_kept == want[k].shape[0]
        np.testing.assert_array_equal(_bits(out[:n_kept]), _bits(want[k]))
        np.testing.assert_array_equal(_bits(out[n_kept:]), _bits(ds[k][held]))
        np.testing.assert_array_equal(index, np.concatenate([np.flatnonzero(~held), np.flatnonzero(held)]))


def test_fixture_covers_the_situations():
    z, _ = load_golden("holdout_ref")
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "holdout_ref.npz")) < 1024 * 1024
    env = "antmaze-umaze-v2"
    ds, want = _case(z, env)
    obs = ds["observations"]
    assert obs.dtype == np.float32 and obs.shape == (HC.N_ROWS, 4) and np.nanmin(obs) >= 0 and np.nanmax(obs) < 32
    at = HC.SPECIAL_AT
    assert obs[at["corner_lo"], :2].tolist() == [5, 2] and obs[at["corner_hi"], :2].tolist() == [10, 7]
    assert obs[at["below_edge"], 0] < 5 and np.nextafter(obs[at["below_edge"], 0], np.float32(np.inf)) == 5
    assert np.isnan(obs[at["nan_x"], 0]) and np.isnan(obs).sum() == 1
    assert obs[at["neg_zero"], 0] == 0 and np.signbit(obs[at["neg_zero"], 0])
    held = HC.held_mask(obs, *HC.box_for(env))
    assert held[at["corner_lo"]] and held[at["corner_hi"]]                         # the inclusive corners are deleted
    assert not held[at["below_edge"]] and not held[at["nan_x"]] and not held[at["neg_zero"]]
    kept_rows = _bits(want["observations"])                                        # ... by the reference itself:
    for name, there in (("corner_lo", False), ("corner_hi", False), ("below_edge", True), ("nan_x", True), ("neg_zero", True)):
        assert (kept_rows == _bits(obs[at[name]])).all(axis=1).any() == there, name
    for e, (lo, hi) in (("antmaze-medium-play-v2", ("medium_lo", "medium_hi")), ("hopper", ("large_lo", "large_hi")),
                        ("antmaze-large-diverse-v2", ("large_lo", "large_hi"))):
        h = HC.held_mask(z[f"{e}/in/observations"], *HC.box_for(e))
        assert h[at[lo]] and h[at[hi]] and z[f"{e}/out/rewards"].size == HC.N_ROWS - h.sum()
    assert HC.box_for("hopper") == HC.box_for("antmaze-large-diverse-v2") == ((26, 30), (14, 18))
    assert HC.box_for("antmaze-umaze-medium") == ((5, 10), (2, 7))                 # "umaze" is tried first
    for name, _, ln in HC.SCORE_CASES:                                             # the scoring cases
        assert z[f"score/{name}/losses"].shape == (3,) and np.isfinite(z[f"score/{name}/losses"]).all()
        keys = [k for k in z.files if k.startswith(f"score/{name}/sd/")]
        assert any("v_target" in k or "v_tgt" in k for k in keys)
        assert any(k.endswith("log_std") for k in keys)
    assert z["score/rows"].shape == (50, 2 * 17 + 2 + 2)


def test_product_boxes_are_the_restated_ones():
    from porl_amd.dataloader import holdout as H
    assert H.HOLDOUT_BOXES == HC.BOXES
    for env in HC.ENV_NAMES + ("antmaze-umaze-medium", ""):
        assert H.box_for(env) == HC.box_for(env)


def test_documented_example():
    rows = np.arange(12, dtype=np.float32).reshape(6, 2)
    held = np.array([0, 1, 1, 0, 0, 1], dtype=np.uint8)
    out, n_kept, index = HC.stable_partition(rows, held)
    assert n_kept == 3 and index.tolist() == [0, 3, 4, 1, 2, 5]
    assert out[:, 0].tolist() == [0, 6, 8, 2, 4, 10]
    obs = np.array([[0.1, 0.5], [np.nextafter(np.float32(0.1), np.float32(0)), 0.5], [0.2, np.nan]], dtype=np.float32)
    assert HC.held_mask(obs, (0.1, 1), (0, 1)).tolist() == [True, False, False]     # 0.1 rounds to fp32 before it is compared
    p = HC.patterns(70, 64)
    assert sorted(p) == ["all", "alternating", "bernoulli", "first", "last", "none", "run"]
    assert np.flatnonzero(p["run"]).tolist() == list(range(61, 68))


def test_abi_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\b(int|int64_t)\s+{name}\s*\(", txt), name
        assert name in N.SYMBOLS
        assert hasattr(N.lib(), name)
    assert re.search(r"typedef struct porl_partition_box\s*\{\s*int32_t cx, cy;[^}]*float x_lo, x_hi, y_lo, y_hi;\s*\}", txt)
    assert C.sizeof(N.PartitionBox) == 24
    assert re.search(r"#define\s+PORL_ABI_VERSION\s+12\b", txt)                    # additions only


def test_tile_constants_are_exported():
    from porl_amd.dataloader.holdout import tile_constants
    T, P = tile_constants()
    assert T >= 64 and P >= 1
    lib = N.lib()
    assert lib.porl_partition_workspace(T, None, None) == 4
    assert lib.porl_partition_workspace(T + 1, None, None) == 6
    assert lib.porl_partition_workspace(T * P + 1, None, None) == 2 + 2 * (P + 1)
    for n in (0, -1, (1 << 36) + 1):
        assert lib.porl_partition_workspace(n, None, None) == -1
        assert "n_rows" in lib.porl_last_error().decode()


# ---- rejected arguments: host buffers, no device -----------------------------------------------------------------------
_F = (C.c_float * 64)()
_O = (C.c_float * 64)()
_M = (C.c_uint8 * 64)()
_I = (C.c_int64 * 64)()
_BOX = N.PartitionBox(0, 1, 5.0, 10.0, 2.0, 7.0)


def _mask(**over):
    a = dict(rows=_F, stride_bytes=16, n_rows=8, row_bytes=16, box=C.pointer(_BOX), mask=_M)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_partition_mask(a["rows"], a["stride_bytes"], a["n_rows"], a["row_bytes"], a["box"], a["mask"], None)
    return rc, lib.porl_last_error().decode()


def _rows(**over):
    a = dict(rows=_F, stride_bytes=16, n_rows=8, row_bytes=16, held=_M, box=None, out=_O, index=_I, workspace=_I)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_partition_rows(a["rows"], a["stride_bytes"], a["n_rows"], a["row_bytes"], a["held"], a["box"], a["out"],
                                 a["index"], a["workspace"], None)
    return rc, lib.porl_last_error().decode()


_CALLS = {"mask": _mask, "rows": _rows}


@pytest.mark.parametrize("fn,arg", [("mask", "rows"), ("mask", "box"), ("mask", "mask"), ("rows", "rows"), ("rows", "out"),
                                    ("rows", "workspace")])
def test_null_pointers_are_rejected_by_name(fn, arg):
    rc, msg = _CALLS[fn](**{arg: None})
    assert rc == -1 and f"null {arg}" in msg, (rc, msg)


@pytest.mark.parametrize("fn,arg,values", [
    ("mask", "n_rows", (0, -1, (1 << 36) + 1)), ("mask", "row_bytes", (0, 6, 18, -16)), ("mask", "stride_bytes", (12, 18, 0, -16)),
    ("rows", "n_rows", (0, -8, (1 << 36) + 1)), ("rows", "row_bytes", (0, 1, 2, 3, 15, -4, (1 << 22) + 4)),
    ("rows", "stride_bytes", (8, 0, 17, -16, (1 << 22) + 4)),
])
def test_bad_sizes_are_rejected_by_name(fn, arg, values):
    for v in values:
        rc, msg = _CALLS[fn](**{arg: v})
        assert rc == -1 and arg in msg, (v, rc, msg)


def test_predicate_forms_are_exclusive():
    rc, msg = _rows(box=C.pointer(_BOX))
    assert rc == -1 and "both" in msg, (rc, msg)
    rc, msg = _rows(held=None)
    assert rc == -1 and "neither" in msg, (rc, msg)
    for field in ("cx", "cy"):
        for v in (4, -1):
            b = N.PartitionBox(0, 1, 5.0, 10.0, 2.0, 7.0)
            setattr(b, field, v)
            for rc, msg in (_rows(held=None, box=C.pointer(b)), _mask(box=C.pointer(b))):
                assert rc == -1 and field in msg, (field, v, rc, msg)


def test_rejected_arguments_under_sanitizers():
    """tests/helpers/abi_reject_holdout.cpp on the host-only sanitized build: every rejected argument of the partition
    entry points comes back as -1 with a message that names it, before any HIP call; ASan / UBSan abort the process on
    any finding.  A stand-alone program: nothing sanitized is loaded into this interpreter."""
    from porl_amd import build as Bd
    assert Bd.build_sanitized_holdout(verbose=False) == Bd.SAN_HOLDOUT_DRIVER
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([Bd.SAN_HOLDOUT_DRIVER], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "0 unexpected" in r.stdout
    n = int(r.stdout.split("abi_reject_holdout:")[1].split("checks")[0])
    assert n >= 45


def test_python_entry_points_have_no_cpu_path():
    import torch
    from porl_amd.buffer.replay_buffer import PackedReplay
    from porl_amd.dataloader import generate_test_generlaization_data, holdout_region, partition_rows
    from porl_amd.util import util as U
    rows = torch.zeros(8, 12)
    held = torch.zeros(8, dtype=torch.uint8)
    ds = {"observations": torch.zeros(8, 4), "rewards": torch.zeros(8)}
    replay = PackedReplay(np.zeros((8, 12), dtype=np.float32), 4, 2, "cpu")
    for call in (lambda: partition_rows(rows, held), lambda: partition_rows(rows, x_range=(0, 1), y_range=(0, 1)),
                 lambda: partition_rows(replay, held), lambda: holdout_region(replay, "antmaze-umaze-v2"),
                 lambda: holdout_region(replay, x_range=(0, 1), y_range=(0, 1)),
                 lambda: generate_test_generlaization_data(dict(ds), "hopper"),
                 lambda: U.generate_test_generlaization_data(dict(ds), "hopper"),
                 lambda: U.generate_test_generlaization_data(replay, "hopper")):
        with pytest.raises(N.NativeError, match="no CPU path"):
            call()
    for bad in (torch.zeros(8, 4, dtype=torch.float16), torch.zeros(8, dtype=torch.uint8), torch.zeros(8, 2, dtype=torch.bool),
                torch.zeros(8, dtype=torch.complex64)):
        with pytest.raises(TypeError, match="dtype"):
            partition_rows(bad, held)
    assert replay.draws == 0


def test_agents_score_on_the_device_only():
    import torch
    from types import SimpleNamespace
    from porl_amd.agent.por import POR, evaluate_store
    from porl_amd.agent.sorl import SORL
    from porl_amd.buffer.replay_buffer import PackedReplay
    args = SimpleNamespace(state_size=6, hidden_dim=16, n_hidden=2, layer_norm=False, action_size=2)
    x, v = torch.zeros(4, 6), torch.zeros(4)
    por, sorl = POR(args, 100, 0.9, 10.0), SORL(args, 100, 0.9, 3.0)
    replay = PackedReplay(np.zeros((8, 16), dtype=np.float32), 6, 2, "cpu")
    for call in (lambda: por.evaluate(x, x, v, v), lambda: sorl.evaluate(x, torch.zeros(4, 2), v, x, v),
                 lambda: por.evaluate_from_replay(replay, 4), lambda: evaluate_store(sorl, replay)):
        with pytest.raises(N.NativeError, match="no CPU path"):
            call()
    assert replay.draws == 0 and por.v_optimizer.step_count == 0 and sorl.policy_optimizer.step_count == 0
