"""The episode passes without a GPU: the numpy restatement (tests/helpers/episode_cases.py) against the reference's
recorded results (tests/golden/episodes_ref.npz, written by tests/helpers/gen_episodes_golden.py), the C ABI's
declaration, and the argument checks of the new entry points, which all come before their first device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden
from helpers import episode_cases as EC
from porl_amd import _native as N

ENTRY_POINTS = ("porl_episode_workspace", "porl_episode_count", "porl_episode_fill", "porl_episode_returns",
                "porl_hindsight_pairs", "porl_gather_pairs")
VECTORS = ("random", "dense", "all_set", "first_only", "last_only", "nan_flag", "neg_zero")


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", VECTORS)
def test_restatement_reproduces_the_reference(name):
    z, _ = load_golden("episodes_ref")
    rew, dones = z[f"{name}_rewards"], z[f"{name}_dones"]
    assert rew.dtype == np.float32 and dones.dtype == np.float32 and rew.size <= 5000
    starts, ends, lengths = EC.extract_done_makers(dones)
    for got, key in ((starts, "starts"), (ends, "ends"), (lengths, "lengths")):
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, z[f"{name}_{key}"])
    s0, e0, trailing = EC.capped_table(dones, 0)                    # the walk without a cap is the same table
    np.testing.assert_array_equal(s0, starts)
    np.testing.assert_array_equal(e0, ends)
    assert trailing == rew.size - 1 - ends[-1]
    for cap, want in zip(EC.CAPS, z[f"{name}_range"]):
        np.testing.assert_array_equal(_bits(EC.return_range(rew, dones, cap)), _bits(want))
        _, lens = EC.episode_returns(rew, dones, cap)
        assert lens.sum() == rew.size and (lens[:-1] <= cap).all() and (lens[:-1] >= 1).all()


def test_fixture_covers_the_situations():
    z, _ = load_golden("episodes_ref")
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "episodes_ref.npz")) < 200 * 1024
    assert np.isnan(z["nan_flag_dones"]).sum() == 1
    nan_at = int(np.flatnonzero(np.isnan(z["nan_flag_dones"]))[0])
    assert nan_at in z["nan_flag_ends"]                            # a NaN flag is set
    nz = z["neg_zero_dones"]
    assert (np.signbit(nz) & (nz == 0)).sum() > 1000               # -0.0 flags, none of them set
    assert z["neg_zero_ends"].size == np.count_nonzero(nz)
    assert z["all_set_lengths"].tolist() == [1] * 300
    assert z["first_only_ends"].tolist() == [0] and z["last_only_ends"].tolist() == [999]
    assert z["random_ends"][-1] < 4999                             # a trailing run the reference drops


def test_documented_examples():
    d = np.array([0, 0, 1, 0, 1, 1, 0, 0], dtype=np.float32)
    r = np.arange(1, 9, dtype=np.float32)
    s, e, l = EC.extract_done_makers(d)
    assert (s.tolist(), e.tolist(), l.tolist()) == ([0, 3, 5], [2, 4, 5], [3, 2, 1])
    assert EC.return_range(r, d, 1000) == (6.0, 9.0)
    assert EC.return_range(r, d, 2) == (3.0, 15.0)
    assert EC.episode_returns(r, d, 2)[1].tolist() == [2, 1, 2, 1, 2, 0]
    assert EC.episode_returns(r, d, 1000)[1].tolist() == [3, 2, 1, 2]
    for out in EC.extract_done_makers(np.zeros(5, dtype=np.float32)):
        assert out.size == 0 and out.dtype == np.int64


@pytest.mark.parametrize("case", [c[0] for c in EC.PAIR_CASES])
def test_pair_restatement_reproduces_the_reference(case):
    z, _ = load_golden("episodes_ref")
    _, vec, _, batch, _ = next(c for c in EC.PAIR_CASES if c[0] == case)
    starts, _, lengths = EC.extract_done_makers(z[f"{vec}_dones"])       # the timeouts when both are present
    traj, u1, u2 = (z[f"pairs_{case}_{k}"] for k in ("traj", "u1", "u2"))
    assert traj.shape == (batch,) and traj.max() < starts.size
    start, goal = EC.pairs_from_draws(starts, lengths, traj, u1, u2)
    np.testing.assert_array_equal(start, z[f"pairs_{case}_start"])
    np.testing.assert_array_equal(goal, z[f"pairs_{case}_goal"])
    assert (start <= goal).all() and (goal <= starts[traj] + lengths[traj] - 1).all()


def test_generator_restatement_is_on_the_grid():
    traj, u1, u2 = EC.device_draws(7, 3, 512, 100003)
    assert traj.min() >= 0 and traj.max() < 100003 and len(set(traj.tolist())) > 500
    for u in (u1, u2):
        assert (u >= 0).all() and (u < 1).all()
        np.testing.assert_array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53))
    assert EC.sm64(0) == 0xE220A8397B1DCDAF                        # splitmix64's first output from state 0
    again = EC.device_draws(7, 3, 512, 100003)
    np.testing.assert_array_equal(traj, again[0])
    assert not np.array_equal(traj, EC.device_draws(7, 4, 512, 100003)[0])


def test_abi_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\b(int|int64_t)\s+{name}\s*\(", txt), name
        assert name in N.SYMBOLS
        assert hasattr(N.lib(), name)
    assert re.search(r"#define\s+PORL_ABI_VERSION\s+12\b", txt)
    assert N.ABI_VERSION == 12 and N.lib().porl_abi_version() == 12


def test_tile_constants_are_exported():
    from porl_amd.dataloader.episodes import tile_constants
    T, P = tile_constants()
    assert T >= 64 and P >= 1
    lib = N.lib()
    assert lib.porl_episode_workspace(T, None, None) == 7
    assert lib.porl_episode_workspace(T + 1, None, None) == 12
    for n in (0, -1, (1 << 40) + 1):
        assert lib.porl_episode_workspace(n, None, None) == -1
        assert "n_rows" in lib.porl_last_error().decode()


# ---- rejected arguments: host buffers, no device -----------------------------------------------------------------------
_F = (C.c_float * 64)()
_D = (C.c_double * 64)()
_I = (C.c_int64 * 64)()


def _count(**over):
    a = dict(flags=_F, stride=1, n_rows=8, cap=0, workspace=_I)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_episode_count(a["flags"], a["stride"], a["n_rows"], a["cap"], a["workspace"], None)
    return rc, lib.porl_last_error().decode()


def _fill(**over):
    a = dict(flags=_F, stride=1, n_rows=8, cap=0, workspace=_I, n_episodes=2, starts=_I, ends=_I)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_episode_fill(a["flags"], a["stride"], a["n_rows"], a["cap"], a["workspace"], a["n_episodes"], a["starts"],
                               a["ends"], None)
    return rc, lib.porl_last_error().decode()


def _returns(**over):
    a = dict(rewards=_F, stride=1, n_rows=8, starts=_I, ends=_I, n_episodes=2, returns=_D, range_ws=_I, range_out=_D)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_episode_returns(a["rewards"], a["stride"], a["n_rows"], a["starts"], a["ends"], a["n_episodes"], a["returns"],
                                  a["range_ws"], a["range_out"], None)
    return rc, lib.porl_last_error().decode()


def _pairs(**over):
    a = dict(starts=_I, lengths=_I, n_episodes=3, batch=8, traj=None, u1=None, u2=None, start=_I, goal=_I)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_hindsight_pairs(a["starts"], a["lengths"], a["n_episodes"], a["batch"], 0, 0, a["traj"], a["u1"], a["u2"],
                                  a["start"], a["goal"], None, None, None, None)
    return rc, lib.porl_last_error().decode()


def _gather(**over):
    a = dict(rows=_F, row_stride=13, n_rows=4, start=_I, goal=_I, batch=2, obs_dim=5, act_dim=1, out=_F, out_stride=13)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_gather_pairs(a["rows"], a["row_stride"], a["n_rows"], a["start"], a["goal"], a["batch"], a["obs_dim"],
                               a["act_dim"], a["out"], a["out_stride"], None)
    return rc, lib.porl_last_error().decode()


_CALLS = {"count": _count, "fill": _fill, "returns": _returns, "pairs": _pairs, "gather": _gather}
_NULLS = [("count", "flags"), ("count", "workspace"),
          ("fill", "flags"), ("fill", "workspace"), ("fill", "starts"), ("fill", "ends"),
          ("returns", "rewards"), ("returns", "starts"), ("returns", "ends"), ("returns", "returns"), ("returns", "range_ws"),
          ("pairs", "starts"), ("pairs", "lengths"), ("pairs", "start"), ("pairs", "goal"),
          ("gather", "rows"), ("gather", "start"), ("gather", "goal"), ("gather", "out")]


@pytest.mark.parametrize("fn,arg", _NULLS)
def test_null_pointers_are_rejected_by_name(fn, arg):
    rc, msg = _CALLS[fn](**{arg: None})
    assert rc == -1 and f"null {arg}" in msg, (rc, msg)


def test_partial_draws_are_rejected_by_name():
    for given, missing in ((dict(u1=_D, u2=_D), "traj"), (dict(traj=_I, u2=_D), "u1"), (dict(traj=_I, u1=_D), "u2")):
        rc, msg = _pairs(**given)
        assert rc == -1 and f"null {missing}" in msg, (rc, msg)


@pytest.mark.parametrize("fn,arg,values", [
    ("count", "n_rows", (0, -1, (1 << 40) + 1)), ("count", "stride", (0, -3)), ("count", "cap", (-1, -(1 << 40))),
    ("fill", "n_rows", (0, (1 << 40) + 1)), ("fill", "stride", (0,)), ("fill", "cap", (-1,)), ("fill", "n_episodes", (0, -1, 9)),
    ("returns", "n_rows", (0, (1 << 40) + 1)), ("returns", "stride", (0, -1)), ("returns", "n_episodes", (0, 9)),
    ("pairs", "n_episodes", (0, -1)), ("pairs", "batch", (0, -5)),
    ("gather", "n_rows", (0, -1)), ("gather", "batch", (0, -1)), ("gather", "obs_dim", (0, -1)), ("gather", "act_dim", (-1,)),
    ("gather", "row_stride", (12, 0, -13)), ("gather", "out_stride", (12, 0)),
])
def test_bad_sizes_are_rejected_by_name(fn, arg, values):
    for v in values:
        rc, msg = _CALLS[fn](**{arg: v})
        assert rc == -1 and arg in msg, (v, rc, msg)


def test_rejected_arguments_under_sanitizers():
    """tests/helpers/abi_reject_episodes.cpp on the host-only sanitized build: every rejected argument of the new entry
    points comes back as -1 with a message that names it, before any HIP call; ASan / UBSan abort the process on any
    finding.  `build_sanitized` keeps returning the first driver."""
    from porl_amd import build as Bd
    assert Bd.build_sanitized(verbose=False) == Bd.SAN_DRIVER
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([Bd.SAN_EPISODES_DRIVER], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "0 unexpected" in r.stdout
    n = int(r.stdout.split("abi_reject_episodes:")[1].split("checks")[0])
    assert n >= 60


def test_python_entry_points_have_no_cpu_path():
    import torch
    from porl_amd.buffer.replay_buffer import PackedReplay
    from porl_amd.dataloader import (EpisodeIndex, episode_returns, extract_done_makers, gather_pairs, hindsight_indices,
                                     return_range, rvs_sample_batch)
    from porl_amd.util import util as U
    d, r = torch.zeros(8), torch.ones(8)
    d[3] = 1
    for call in (lambda: extract_done_makers(d), lambda: EpisodeIndex.from_dones(d), lambda: episode_returns(r, d, 10),
                 lambda: return_range({"rewards": r, "terminals": d}, 10), lambda: U.extract_done_makers(d),
                 lambda: U.return_range({"rewards": r, "terminals": d}, 10),
                 lambda: gather_pairs(torch.zeros(4, 12), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 4, 2)):
        with pytest.raises(N.NativeError, match="no CPU path"):
            call()
    rows = np.zeros((8, 12), dtype=np.float32)
    rows[:, 9] = 1
    replay = PackedReplay(rows, 4, 2, "cpu")
    for call in (lambda: rvs_sample_batch(replay, 4), lambda: U.rvs_sample_batch(replay, 4), lambda: return_range(replay, 10),
                 lambda: EpisodeIndex.from_replay(replay)):
        with pytest.raises(N.NativeError, match="no CPU path"):
            call()
    assert replay.draws == 0
    ix = EpisodeIndex(torch.tensor([0]), torch.tensor([3]), 8, 4)
    assert ix.lengths.tolist() == [4] and ix.n_episodes == 1 and len(ix) == 1
    with pytest.raises(N.NativeError, match="no CPU path"):
        hindsight_indices(ix, 4)
    with pytest.raises(ValueError, match="max_episode_steps"):     # checked before the device is
        return_range({"rewards": r, "terminals": d}, 0)
