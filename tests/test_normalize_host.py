"""Dataset normalisation without a GPU: the numpy restatement (tests/helpers/normalize_cases.py) and `ColumnStats.merge`
against the fsum oracle inside the derived bounds, two negative controls that must miss them, the Normalizer's host
arithmetic, the C ABI's declaration, and the argument checks of the new entry points, which all come before their first
device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from helpers import normalize_cases as NC
from porl_amd import _native as N
from porl_amd.dataloader import ColumnStats, Normalizer, column_stats, normalize_dataset
from porl_amd.dataloader.normalize import tile_constants
import porl_amd.ops  # noqa: F401  (registers torch.ops.porl_hip)

ENTRY_POINTS = ("porl_colstats_workspace", "porl_col_stats", "porl_affine_cols")


@pytest.fixture(scope="module")
def columns():
    """case -> (x, oracle, (mean bound, var bound)) at N = 70 001, computed once."""
    rng = np.random.default_rng(11)
    out = {}
    for case in NC.CASES:
        x = NC.column(case, NC.HOST_N, rng)
        out[case] = (x, NC.oracle(x), NC.bounds(x) if case in NC.FINITE else None)
    return out


def _inside(case, got_mean, got_m2, got_min, got_max, x, want, bound):
    n = x.size
    mean, m2, lo, hi = want
    dm, dv = abs(got_mean - mean), abs(got_m2 / n - m2 / n)
    print(f"{case}: |d mean| = {dm:.3e} (bound {bound[0]:.3e}), |d var| = {dv:.3e} (bound {bound[1]:.3e})")
    assert dm <= bound[0], (case, dm, bound[0])
    assert dv <= bound[1], (case, dv, bound[1])
    assert got_min == lo and got_max == hi, case


@pytest.mark.parametrize("case", NC.FINITE)
def test_tile_merged_restatement_is_inside_the_bounds(columns, case):
    T, P = tile_constants()
    x, want, bound = columns[case]
    n, mean, m2, lo, hi = NC.tile_merged(x, T, P)
    assert n == x.size
    _inside(case, mean, m2, lo, hi, x, want, bound)
    if case == "const":
        assert m2 == 0.0


@pytest.mark.parametrize("shards", (1, 2, 7))
@pytest.mark.parametrize("case", NC.FINITE)
def test_column_stats_merge_of_unequal_shards(columns, case, shards):
    T, P = tile_constants()
    x, want, bound = columns[case]
    cuts = [0] + sorted(np.random.default_rng(shards).choice(np.arange(1, x.size), size=shards - 1, replace=False).tolist()) + [x.size]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        n, mean, m2, lo, hi = NC.tile_merged(x[a:b], T, P)
        parts.append(ColumnStats(n, [mean], [m2], [lo], [hi]))
    assert len({p.n for p in parts}) == len(parts)                 # unequal
    got = parts[0].merge(*parts[1:])
    assert got.n == x.size and got.mean.dtype == np.float64
    _inside(case, got.mean[0], got.m2[0], got.min[0], got.max[0], x, want, bound)
    np.testing.assert_array_equal(got.var, got.m2 / x.size)
    np.testing.assert_array_equal(got.std, np.sqrt(got.m2 / x.size))
    if case == "const":
        assert got.m2[0] == 0.0


def test_merge_carries_nan_and_rejects_other_widths(columns):
    a = ColumnStats(3, [1.0, 2.0], [0.5, 0.5], [0.0, np.nan], [2.0, np.nan])
    b = ColumnStats(2, [1.0, np.nan], [0.0, np.nan], [1.0, 1.0], [1.0, 1.0])
    got = a.merge(b)
    assert got.n == 5 and got.mean[0] == 1.0 and got.m2[0] == 0.5 and (got.min[0], got.max[0]) == (0.0, 2.0)
    assert np.isnan([got.mean[1], got.m2[1], got.min[1], got.max[1]]).all()
    with pytest.raises(ValueError, match="columns"):
        a.merge(ColumnStats(1, [0.0], [0.0], [0.0], [0.0]))


def test_negative_controls_miss_the_bounds(columns):
    """The bounds bite: the one-pass sum x^2 form in fp64 misses `offset`'s variance and gives a non-zero variance on
    `const`; fp32 accumulation misses on `gauss`."""
    x, (mean, m2, _, _), bound = columns["offset"]
    _, var = NC.one_pass(x)
    print(f"one-pass offset: |d var| = {abs(var - m2 / x.size):.3e} (bound {bound[1]:.3e})")
    assert abs(var - m2 / x.size) > bound[1]
    x, (mean, m2, _, _), bound = columns["const"]
    _, var = NC.one_pass(x)
    print(f"one-pass const: var = {var:.3e} (oracle {m2 / x.size})")
    assert m2 == 0.0 and bound[1] == 0.0 and var != 0.0
    x, (mean, m2, _, _), bound = columns["gauss"]
    m32, v32 = NC.fp32_accumulation(x)
    print(f"fp32 gauss: |d mean| = {abs(m32 - mean):.3e} (bound {bound[0]:.3e}), |d var| = {abs(v32 - m2 / x.size):.3e} (bound {bound[1]:.3e})")
    assert abs(v32 - m2 / x.size) > bound[1]                        # (its mean, rounded once to fp32, can land inside by luck)


def test_normalizer_from_stats(columns):
    names = list(NC.FINITE)
    st = [columns[c][1] for c in names]
    n = NC.HOST_N
    stats = ColumnStats(n, [s[0] for s in st], [s[1] for s in st], [s[2] for s in st], [s[3] for s in st])
    for eps in (1e-3, 0.0, 0.25):
        norm = Normalizer.from_stats(stats, eps=eps)
        mean32, std32 = NC.normalizer_from_stats(n, stats.mean, stats.m2, eps)
        assert norm.mean.dtype == norm.std.dtype == torch.float32 and norm.mean.device.type == "cpu"
        np.testing.assert_array_equal(norm.mean.numpy().view(np.int32), mean32.view(np.int32))
        np.testing.assert_array_equal(norm.std.numpy().view(np.int32), std32.view(np.int32))
        assert norm.std[names.index("const")].item() == np.float32(eps)          # std of a constant column is eps itself
    assert norm.obs_dim == len(names) and norm.reward_div is None and norm.reward_mul is None
    for case in ("nan1", "inf1"):
        o = columns[case][1]
        bad = ColumnStats(n, [0.0, 0.0, o[0]], [1.0, 1.0, o[1]], [0.0, 0.0, o[2]], [0.0, 0.0, o[3]])
        with pytest.raises(ValueError, match="column 2"):
            Normalizer.from_stats(bad)


def test_reward_scale():
    norm = Normalizer(np.zeros(3, dtype=np.float32), np.ones(3, dtype=np.float32))
    with pytest.raises(ValueError, match="max return == min return"):
        norm.with_reward_scale(2.5, 2.5, 1000)
    assert norm.reward_div is None
    assert norm.with_reward_scale(-0.1, 0.2, 1000) is norm
    assert norm.reward_div == float(np.float32(0.2 - -0.1)) and norm.reward_mul == 1000.0
    with pytest.raises(ValueError, match="together"):
        Normalizer(np.zeros(3), np.ones(3), reward_div=2.0)


def test_state_dict_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    norm = Normalizer(rng.standard_normal(5).astype(np.float32), rng.uniform(0.5, 2, 5).astype(np.float32))
    norm.with_reward_scale(-3.25, 11.0, 700)
    path = tmp_path / "norm.pt"
    torch.save({"normalizer": norm.state_dict()}, path)
    sd = torch.load(path, weights_only=True)["normalizer"]
    back = Normalizer(np.zeros(5), np.ones(5)).load_state_dict(sd)
    assert torch.equal(back.mean, norm.mean) and torch.equal(back.std, norm.std)
    assert (back.reward_div, back.reward_mul) == (norm.reward_div, norm.reward_mul) == (float(np.float32(14.25)), 700.0)
    plain = Normalizer(np.zeros(5), np.ones(5)).load_state_dict(Normalizer(norm.mean, norm.std).state_dict())
    assert plain.reward_div is None and plain.reward_mul is None
    assert back.to("cpu") is back


def test_abi_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\b(int|int64_t)\s+{name}\s*\(", txt), name
        assert name in N.SYMBOLS
        assert hasattr(N.lib(), name)
    assert re.search(r"typedef struct porl_col_span\s*\{\s*int32_t col0, n_cols, param0, flags;\s*\}\s*porl_col_span;", txt)
    assert C.sizeof(N.ColSpan) == 16
    assert re.search(r"#define\s+PORL_ABI_VERSION\s+12\b", txt)                    # additions only
    assert N.ABI_VERSION == 12 and N.lib().porl_abi_version() == 12


def test_workspace_sizes():
    T, P = tile_constants()
    assert T >= 64 and P >= 2
    lib = N.lib()
    K = lib.porl_colstats_workspace(1, 1, None, None)             # doubles per column of a stored partial
    assert K >= 4
    for c in (1, 60, 4096):
        assert lib.porl_colstats_workspace(1, c, None, None) == K * c
        assert lib.porl_colstats_workspace(T, c, None, None) == K * c
        assert lib.porl_colstats_workspace(T + 1, c, None, None) == K * c * 2
        assert lib.porl_colstats_workspace(T * P, c, None, None) == K * c * P
        assert lib.porl_colstats_workspace(T * P + 1, c, None, None) == K * c * (P + 1 + 2)     # a second level of 2
        assert lib.porl_colstats_workspace(T * P * P + 1, c, None, None) == K * c * (P * P + 1 + P + 1 + 2)
    for n in (0, -1, (1 << 36) + 1):
        assert lib.porl_colstats_workspace(n, 3, None, None) == -1
        assert "n_rows" in lib.porl_last_error().decode()
    for c in (0, 4097):
        assert lib.porl_colstats_workspace(8, c, None, None) == -1
        assert "n_cols" in lib.porl_last_error().decode()
    assert lib.porl_colstats_workspace(1 << 36, 4096, None, None) > 0


# ---- rejected arguments: host buffers, no device -----------------------------------------------------------------------
_F = (C.c_float * 256)()
_O = (C.c_float * 256)()
_D = (C.c_double * 256)()
_W = (C.c_double * 256)()
_P = (C.c_float * 16)()


def _stats(**over):
    a = dict(rows=_F, stride_floats=12, n_rows=8, col0=0, n_cols=4, workspace=_W, out=_D)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_col_stats(a["rows"], a["stride_floats"], a["n_rows"], a["col0"], a["n_cols"], a["workspace"], a["out"], None)
    return rc, lib.porl_last_error().decode()


def _spans(*s):
    return (N.ColSpan * len(s))(*[N.ColSpan(*v) for v in s])


def _affine(**over):
    a = dict(rows=_F, stride_floats=12, n_rows=8, width=12, spans=_spans((0, 4, 0, 0), (5, 4, 0, 0)), n_spans=2, shift=_P, div=_P,
             mul=_P, n_params=5, out=_O, out_stride_floats=12)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_affine_cols(a["rows"], a["stride_floats"], a["n_rows"], a["width"], a["spans"], a["n_spans"], a["shift"],
                              a["div"], a["mul"], a["n_params"], a["out"], a["out_stride_floats"], None)
    return rc, lib.porl_last_error().decode()


_CALLS = {"stats": _stats, "affine": _affine}


@pytest.mark.parametrize("fn,arg", [("stats", "rows"), ("stats", "workspace"), ("stats", "out"), ("affine", "rows"),
                                    ("affine", "out"), ("affine", "spans"), ("affine", "shift"), ("affine", "div")])
def test_null_pointers_are_rejected_by_name(fn, arg):
    rc, msg = _CALLS[fn](**{arg: None})
    assert rc == -1 and f"null {arg}" in msg, (rc, msg)


@pytest.mark.parametrize("fn,arg,values", [
    ("stats", "n_rows", (0, -1, (1 << 36) + 1)), ("stats", "n_cols", (0, -4, 4097)), ("stats", "col0", (-1, 1 << 20)),
    ("stats", "stride_floats", (3, 0, -12, (1 << 20) + 4)),
    ("affine", "n_rows", (0, -8, (1 << 36) + 1)), ("affine", "width", (0, -1, (1 << 20) + 1)),
    ("affine", "stride_floats", (11, 0, -12, (1 << 20) + 4)), ("affine", "out_stride_floats", (11, 0, -12, (1 << 20) + 4)),
    ("affine", "n_spans", (0, 9, -1)), ("affine", "n_params", (0, -1)),
])
def test_bad_sizes_are_rejected_by_name(fn, arg, values):
    for v in values:
        rc, msg = _CALLS[fn](**{arg: v})
        assert rc == -1 and arg in msg, (v, rc, msg)


def test_bad_spans_are_rejected_by_name():
    rc, msg = _stats(col0=9)                                        # col0 + n_cols = 13 > stride 12
    assert rc == -1 and "stride_floats" in msg, (rc, msg)
    for spans, word in ((((0, 4, 0, 0), (3, 4, 0, 0)), "overlap"), (((5, 4, 0, 0), (3, 3, 0, 0)), "overlap"),
                        (((0, 4, 0, 0), (9, 4, 0, 0)), "width"), (((0, 13, 0, 0),), "width"), (((-1, 2, 0, 0),), "width"),
                        (((0, 0, 0, 0),), "width"), (((0, 4, 2, 0),), "n_params"), (((0, 4, -1, 0),), "n_params"),
                        (((0, 6, 0, 0),), "n_params"), (((0, 4, 0, 2),), "flags")):
        rc, msg = _affine(spans=_spans(*spans), n_spans=len(spans))
        assert rc == -1 and word in msg, (spans, rc, msg)
    rc, msg = _affine(spans=_spans((0, 4, 0, 0), (4, 1, 4, 1)), mul=None)
    assert rc == -1 and "null mul" in msg, (rc, msg)
    rc, msg = _affine(out=_F, out_stride_floats=16)                 # in place needs one stride
    assert rc == -1 and "out_stride_floats" in msg, (rc, msg)


def test_rejected_arguments_under_sanitizers():
    """tests/helpers/abi_reject_normalize.cpp on the host-only sanitized build: every rejected argument of the three entry
    points comes back as -1 with a message that names it, before any HIP call; ASan / UBSan abort the process on any
    finding.  A stand-alone program: nothing sanitized is loaded into this interpreter."""
    from porl_amd import build as Bd
    assert Bd.build_sanitized_normalize(verbose=False) == Bd.SAN_NORMALIZE_DRIVER
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([Bd.SAN_NORMALIZE_DRIVER], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "0 unexpected" in r.stdout
    n = int(r.stdout.split("abi_reject_normalize:")[1].split("checks")[0])
    assert n >= 40


def test_python_entry_points_have_no_cpu_path():
    from porl_amd.agent.policy import GaussianPolicy
    from porl_amd.buffer.replay_buffer import PackedReplay
    from porl_amd.util import util as U
    rows = torch.zeros(8, 12)
    replay = PackedReplay(np.zeros((8, 12), dtype=np.float32), 4, 2, "cpu")
    norm = Normalizer(np.zeros(4, dtype=np.float32), np.ones(4, dtype=np.float32))
    for call in (lambda: column_stats(rows), lambda: column_stats(replay), lambda: column_stats(rows, (1, 3)),
                 lambda: norm.apply(torch.zeros(3, 4)), lambda: norm.apply(torch.zeros(4)), lambda: norm.apply_(rows),
                 lambda: norm.apply_(replay), lambda: normalize_dataset(replay), lambda: normalize_dataset(replay, 5),
                 lambda: torch.ops.porl_hip.col_stats(rows, 0, 4),
                 lambda: torch.ops.porl_hip.affine_cols(rows, [0, 4, 0, 0], norm.mean, norm.std, None)):
        with pytest.raises(N.NativeError, match="no CPU"):
            call()
    assert getattr(replay, "normalizer", None) is None
    env = NC.ScriptedEnv()
    pol, goal = GaussianPolicy(NC.EVAL_S, NC.EVAL_A, 16, 2), GaussianPolicy(NC.EVAL_S, NC.EVAL_S, 16, 2)
    pol2 = GaussianPolicy(2 * NC.EVAL_S, NC.EVAL_A, 16, 2)
    mean, std = NC.eval_mean_std()
    for call in (lambda: U.evaluate_iql(env, pol, mean, std), lambda: U.evaluate_por(env, pol2, goal, mean, std),
                 lambda: U.evaluate_rvs(env, pol, mean, std), lambda: U.evaluate_iql(env, pol, norm)):
        with pytest.raises(N.NativeError, match="no CPU path"):
            call()
    assert env.t == 0 and env.actions == []                         # refused before the first step


def test_a_normalised_store_is_refused_before_any_native_call():
    from porl_amd.buffer.replay_buffer import PackedReplay
    replay = PackedReplay(np.zeros((8, 12), dtype=np.float32), 4, 2, "cpu")
    replay.normalizer = Normalizer(np.zeros(4, dtype=np.float32), np.ones(4, dtype=np.float32))
    with pytest.raises(ValueError, match="already has a normalizer"):      # a CPU store: a native call would say "no CPU path"
        normalize_dataset(replay, 10)
