"""CPU-side checks of the row-source entry points (porl_enc_forward_rows, porl_iql_load_batch_indexed) and of the Python
checks of `update_from_replay` that need no device: the ctypes table against the header, the refusals made before
anything is launched, and the rejected-argument paths of the two entry points under ASan + UBSan in a stand-alone
driver (tests/helpers/abi_reject_rows.cpp)."""
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO
from porl_amd import _native as N
from porl_amd.util.synth import make_rows

NEW = ("porl_enc_forward_rows", "porl_iql_load_batch_indexed")


def _header_prototype(name):
    txt = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_ctypes_table_matches_the_header():
    lib = N.lib()
    for name in NEW:
        assert name in N.SYMBOLS
        params = _header_prototype(name)
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, params)
        # pointers are passed as void*, the integer widths are the header's
        for p, t in zip(params, fn.argtypes):
            want = N.C.c_void_p if "*" in p else {"int32_t": N.C.c_int32, "int64_t": N.C.c_int64}[p.split()[0]]
            assert t is want, (name, p, t)
    assert lib.porl_abi_version() == N.ABI_VERSION == 12


def test_signatures():
    import inspect
    from porl_amd.agent.fasternet import FasterNet
    from porl_amd.agent.por import POR
    from porl_amd.agent.sorl import SORL
    from porl_amd.engine import IqlEngine
    for cls in (POR, SORL):
        sig = inspect.signature(cls.update_from_replay)
        assert list(sig.parameters) == ["agent", "replay", "batch_size", "indices"] and sig.parameters["indices"].default is None
    sig = inspect.signature(FasterNet.forward_rows)
    assert list(sig.parameters) == ["self", "rows", "idx", "col_offset", "drop_scale"]
    assert sig.parameters["col_offset"].default == 0 and sig.parameters["drop_scale"].default is None
    assert callable(IqlEngine.load_batch_indexed)


def _args(S, A=2, B=4):
    return SimpleNamespace(state_size=S, feature_dim=64, hidden_dim=64, n_hidden=2, layer_norm=False, action_size=A, max_batch=B)


def _cpu_agents():
    """(agent, its raw state width, its scheduler) for a heads-only POR and a SORL with a backbone, all on the CPU: the
    checks below are made before the first native call, so no device is needed."""
    from porl_amd.agent.fasternet import FasterNet
    from porl_amd.agent.por import POR
    from porl_amd.agent.sorl import SORL
    torch.manual_seed(0)
    por = POR(_args(60), 100, 0.9, 10.0)
    bb = FasterNet(3, 64, max_batch=4, angle_bins=40, dist_bins=64)
    sorl = SORL(_args(42), 100, 0.9, 3.0, backbone=bb)
    return [(por, 60, por.goal_lr_schedule), (sorl, 42, sorl.lr_schedule)]


def test_python_refusals_need_no_device_and_count_nothing():
    from porl_amd.buffer.replay_buffer import PackedReplay
    for agent, S, sched in _cpu_agents():
        B, A, N_ = 4, 2, 12
        replay = PackedReplay(make_rows(N_, S, A, seed=1), S, A, "cpu")
        narrow = PackedReplay(make_rows(N_, S - 1, A, seed=1), S - 1, A, "cpu")
        good = torch.arange(B, dtype=torch.int64)
        opts = [agent.v_optimizer, getattr(agent, "policy_optimizer", None) or agent.goal_policy_optimizer]
        with pytest.raises(ValueError) as ei:
            agent.update_from_replay(narrow, B)
        assert str(S - 1) in str(ei.value) and str(S) in str(ei.value)          # both widths are named
        with pytest.raises(ValueError):
            agent.update_from_replay(narrow, B, indices=good)
        with pytest.raises(RuntimeError, match="int64"):
            agent.update_from_replay(replay, B, indices=good.to(torch.int32))
        with pytest.raises(RuntimeError, match="shape"):
            agent.update_from_replay(replay, B, indices=good[:3])
        with pytest.raises(RuntimeError, match="shape"):
            agent.update_from_replay(replay, B, indices=good.view(2, 2))
        with pytest.raises(RuntimeError, match="meta"):
            agent.update_from_replay(replay, B, indices=torch.empty(B, dtype=torch.int64, device="meta"))   # another device
        with pytest.raises(RuntimeError, match="max_batch"):
            agent.update_from_replay(replay, B + 1, indices=torch.arange(B + 1, dtype=torch.int64))
        with pytest.raises(N.NativeError, match="no CPU path"):                  # accepted arguments: refused by the engine
            agent.update_from_replay(replay, B, indices=good)
        assert replay.draws == 0 and narrow.draws == 0 and sched.last_epoch == 0
        assert [o.step_count for o in opts] == [0, 0]
        if getattr(agent, "backbone", None) is not None:
            assert all(int(v) == 0 for k, v in agent.backbone.state_dict().items() if k.endswith("num_batches_tracked"))


def test_phase_forms_check_the_store_too():
    from porl_amd.buffer.replay_buffer import PackedReplay
    agent, S, _ = _cpu_agents()[1]
    narrow = PackedReplay(make_rows(12, S - 1, 2, seed=1), S - 1, 2, "cpu")
    for call in (agent.vf_update_from_replay, agent.policy_update_from_replay):
        with pytest.raises(ValueError):
            call(narrow, 4)
        with pytest.raises(NotImplementedError):
            call(None, 4)                                        # with a backbone the rows must lie in a PackedReplay
    assert narrow.draws == 0


def test_forward_rows_checks_its_arguments():
    from porl_amd.agent.fasternet import FasterNet
    m = FasterNet(3, 64, max_batch=4, angle_bins=40, dist_bins=64)
    with pytest.raises(N.NativeError, match="no CPU path"):
        m.forward_rows(torch.zeros(5, 86), torch.zeros(2, dtype=torch.int64))


def test_rejected_arguments_under_sanitizers():
    """tests/helpers/abi_reject_rows.cpp on the host-only sanitized build: every rejected argument of the two entry
    points comes back as a non-zero status with a message that names it, before any HIP call; ASan / UBSan abort the
    process on any finding."""
    from porl_amd import build as Bd
    Bd.build_sanitized(verbose=False)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([Bd.SAN_ROWS_DRIVER], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "0 unexpected" in r.stdout
    n = int(r.stdout.split("abi_reject_rows:")[1].split("checks")[0])
    assert n >= 40
