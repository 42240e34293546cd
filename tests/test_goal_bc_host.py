"""The goal-conditioned behaviour-cloning entry points without a device: what the header declares, every rejected
argument by name (through ctypes with host buffers, and in a stand-alone program under the host sanitizers), and the
Python layer's refusal to run on the CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from porl_amd import _native as N

ENTRY_POINTS = ("porl_iql_load_batch_cat", "porl_iql_load_batch_pairs", "porl_iql_bc_forward", "porl_iql_bc_step")


def test_abi_declares_the_entry_points():
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint\s+{name}\s*\(", txt), name
        assert name in N.SYMBOLS
        assert hasattr(N.lib(), name)
    assert re.search(r"#define\s+PORL_ABI_VERSION\s+12\b", txt)                    # additions only
    assert N.ABI_VERSION == 12 and N.lib().porl_abi_version() == 12


# ---- rejected arguments: a bound engine over host buffers, no device ------------------------------------------------------
S, G, A, W = 60, 60, 2, 124
_X = (C.c_float * 256)()
_I = (C.c_int64 * 128)()


@pytest.fixture(scope="module")
def eng():
    """pi(a | s, g) for 60-wide states and goals, 2 actions, bound to host memory: bind only records the pointers, and every
    call below is refused before it would touch them."""
    lib = N.lib()
    cfg = N.IqlCfg(S + G, A, 64, 2, 0, 0, 1, 128)
    h = C.c_void_p()
    assert lib.porl_iql_create(C.byref(cfg), C.byref(h)) == 0
    nv, npol, nw = lib.porl_iql_group_floats(h, 0), lib.porl_iql_group_floats(h, 1), lib.porl_iql_workspace_floats(h)
    keep = [np.zeros(n + 16, np.float32) for n in (nv, nv, npol, nv, npol, nv, nv, npol, npol, nw, 8)]
    ptrs = [(a.ctypes.data + 15) // 16 * 16 for a in keep]
    bufs = N.IqlBuffers(*[C.c_void_p(p) for p in ptrs])
    assert lib.porl_iql_bind(h, C.byref(bufs)) == 0
    yield h
    lib.porl_iql_destroy(h)
    del keep


def _cat(h, **over):
    a = dict(batch=8, obs=_X, obs_rs=S, goals=_X, goals_rs=G, goal_dim=G, actions=_X, act_rs=A)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_iql_load_batch_cat(h, a["batch"], a["obs"], a["obs_rs"], a["goals"], a["goals_rs"], a["goal_dim"], a["actions"],
                                     a["act_rs"], None)
    return rc, lib.porl_last_error().decode()


def _pairs(h, **over):
    a = dict(batch=8, rows=_X, row_stride=W, n_rows=100, state_dim=S, act_dim=A, goal_col=S + 1, goal_dim=G, start=_I, goal=_I,
             ep_starts=None, ep_lengths=None, n_episodes=0)
    a.update(over)
    lib = N.lib()
    rc = lib.porl_iql_load_batch_pairs(h, a["batch"], a["rows"], a["row_stride"], a["n_rows"], a["state_dim"], a["act_dim"],
                                       a["goal_col"], a["goal_dim"], a["start"], a["goal"], a["ep_starts"], a["ep_lengths"],
                                       a["n_episodes"], 1, 2, None, None, None)
    return rc, lib.porl_last_error().decode()


_CALLS = {"cat": _cat, "pairs": _pairs}


@pytest.mark.parametrize("fn,arg", [("cat", "obs"), ("cat", "goals"), ("cat", "actions"), ("pairs", "rows")])
def test_null_pointers_are_rejected_by_name(eng, fn, arg):
    rc, msg = _CALLS[fn](eng, **{arg: None})
    assert rc == -1 and f"null {arg}" in msg, (rc, msg)


def test_null_or_unbound_engine_is_rejected():
    lib = N.lib()
    hp = N.IqlHyper()
    cfg = N.IqlCfg(S + G, A, 64, 2, 0, 0, 1, 128)
    h = C.c_void_p()
    assert lib.porl_iql_create(C.byref(cfg), C.byref(h)) == 0
    try:
        for rc in (_cat(None)[0], _pairs(None)[0], lib.porl_iql_bc_step(None, C.byref(hp), None),
                   lib.porl_iql_bc_forward(None, C.byref(hp), None)):
            assert rc == -1 and "null engine" in lib.porl_last_error().decode()
        for call in (lambda: _cat(h)[0], lambda: _pairs(h)[0], lambda: lib.porl_iql_bc_step(h, C.byref(hp), None),
                     lambda: lib.porl_iql_bc_forward(h, C.byref(hp), None)):
            assert call() == -3 and "bind" in lib.porl_last_error().decode()
    finally:
        lib.porl_iql_destroy(h)


@pytest.mark.parametrize("fn,arg,values", [
    ("cat", "batch", (0, 129, -4)), ("cat", "goal_dim", (0, -1, 120, 2 ** 31 - 1)), ("cat", "obs_rs", (59, 0, -60)),
    ("cat", "goals_rs", (59, -60)), ("cat", "act_rs", (1, 0)),
    ("pairs", "batch", (0, 129, -1)), ("pairs", "n_rows", (0, -7, (1 << 40) + 1)), ("pairs", "state_dim", (0, -3)),
    ("pairs", "act_dim", (0, -1)), ("pairs", "goal_dim", (0, -2)),
    ("pairs", "row_stride", (123, 0, -124, 2 ** 63 - 1)),           # shorter than 2S + 2 + A
    ("pairs", "goal_col", (-1, 63, 2 ** 31 - 1)),                  # negative; 63 + 60 > 2S + 2: past the state part of a row
])
def test_bad_sizes_are_rejected_by_name(eng, fn, arg, values):
    for v in values:
        rc, msg = _CALLS[fn](eng, **{arg: v})
        assert rc == -1 and arg in msg, (v, rc, msg)


def test_widths_must_be_the_engines(eng):
    rc, msg = _pairs(eng, goal_col=0, goal_dim=2)                              # 60 + 2 != cfg.obs_dim
    assert rc == -1 and "obs_dim" in msg and "state_dim 60 + goal_dim 2" in msg, (rc, msg)
    rc, msg = _pairs(eng, act_dim=3, row_stride=125)                           # != cfg.pol_out_dim
    assert rc == -1 and "pol_out_dim" in msg and "act_dim 3" in msg, (rc, msg)


def test_index_modes_are_exclusive_and_complete(eng):
    rc, msg = _pairs(eng, start=None)                                          # a goal without a start
    assert rc == -1 and "null start" in msg, (rc, msg)
    rc, msg = _pairs(eng, start=None, goal=None, ep_starts=_I, n_episodes=4)   # only one of the two table pointers
    assert rc == -1 and "ep_lengths is null" in msg, (rc, msg)
    rc, msg = _pairs(eng, start=None, goal=None, ep_lengths=_I, n_episodes=4)
    assert rc == -1 and "ep_starts is null" in msg, (rc, msg)
    for n in (0, -2, 101):
        rc, msg = _pairs(eng, start=None, goal=None, ep_starts=_I, ep_lengths=_I, n_episodes=n)
        assert rc == -1 and "n_episodes" in msg, (n, rc, msg)
    rc, msg = _pairs(eng, goal=None, ep_starts=_I, ep_lengths=_I, n_episodes=4)          # a table AND start rows
    assert rc == -1 and "both given" in msg, (rc, msg)
    rc, msg = _pairs(eng, start=None, goal=None, n_rows=7)                     # 8 distinct rows of 7
    assert rc == -1 and "n_rows" in msg, (rc, msg)


def test_the_step_needs_a_staged_batch(eng):
    lib = N.lib()
    hp = N.IqlHyper()
    for name in ("porl_iql_bc_step", "porl_iql_bc_forward", "porl_iql_policy_backward"):
        assert getattr(lib, name)(eng, C.byref(hp), None) == -1
        assert "no minibatch loaded" in lib.porl_last_error().decode()


def test_rejected_arguments_under_sanitizers():
    """tests/helpers/abi_reject_goal_bc.cpp on the host-only sanitized build: every rejected argument of the four entry
    points comes back as an error code with a message that names it, before any HIP call; ASan / UBSan abort the process on
    any finding.  A stand-alone program: nothing sanitized is loaded into this interpreter."""
    from porl_amd import build as Bd
    assert Bd.build_sanitized_goal_bc(verbose=False) == Bd.SAN_GOAL_BC_DRIVER
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([Bd.SAN_GOAL_BC_DRIVER], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "0 unexpected" in r.stdout
    n = int(r.stdout.split("abi_reject_goal_bc:")[1].split("checks")[0])
    assert n >= 40


def test_python_entry_points_have_no_cpu_path():
    import torch
    from types import SimpleNamespace
    from porl_amd.agent import GoalConditionedBC
    from porl_amd.agent.por import POR
    from porl_amd.buffer.replay_buffer import PackedReplay
    bc = GoalConditionedBC(6, 6, 2, 100, hidden_dim=16, max_batch=8)
    o, g, a = torch.zeros(4, 6), torch.zeros(4, 6), torch.zeros(4, 2)
    replay = PackedReplay(np.zeros((8, 16), dtype=np.float32), 6, 2, "cpu")
    idx = torch.arange(4)
    for call in (lambda: bc.update(o, g, a), lambda: bc.evaluate(o, g, a), lambda: bc.update_from_replay(replay, 4),
                 lambda: bc.update_from_replay(replay, 4, goal="hindsight"),
                 lambda: bc.update_from_replay(replay, 4, indices=idx), lambda: bc.evaluate_from_replay(replay, 4),
                 lambda: bc.evaluate_store(replay), lambda: bc._engine.load_batch_cat(o, g, a),
                 lambda: bc._engine.load_batch_pairs(replay.rows, 4, 6, 2, 7, 6)):
        with pytest.raises(N.NativeError, match="no CPU path"):
            call()
    with pytest.raises(N.NativeError, match="no CPU path"):
        bc.update(o, g, a)
    assert replay.draws == 0 and bc.policy_optimizer.step_count == 0 and bc.policy_lr_schedule.last_epoch == 0
    # POR acts through it: outside the module registry, and only once it is set
    args = SimpleNamespace(state_size=6, hidden_dim=16, n_hidden=2, layer_norm=False, action_size=2)
    por = POR(args, 100, 0.9, 10.0)
    keys = list(por.state_dict().keys())
    assert len(keys) == 31
    with pytest.raises(RuntimeError, match="set_execute_policy"):
        por.select_action(np.zeros(6, np.float32))
    por.set_execute_policy(bc)
    assert list(por.state_dict().keys()) == keys and bc not in list(por.modules())
    with pytest.raises(TypeError):
        por.set_execute_policy(bc.policy)
    with pytest.raises(ValueError):
        por.set_execute_policy(GoalConditionedBC(6, 2, 2, 100, hidden_dim=16))
