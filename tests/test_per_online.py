"""CPU-side checks of the prioritized-replay online path: the golden run of the reference's PERTrainer.train_online
(scripts/gen_golden_online_per.py) stayed clear of every decision a rounding difference could flip, and the three
entry points behind PrioritizedReplayBuffer.record / sample_slots / update_priorities_device turn bad arguments down
before anything is launched (so no GPU is needed to see it)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from porl_amd import _native as N


def test_golden_run_is_well_separated():
    z, _ = load_golden("online_per_s8_a4")
    assert float(z["min_gap"]) >= 1e-3                   # no greedy choice near a tie
    assert float(z["min_margin"]) >= 5e-5                # no tree-walk comparison near its boundary
    assert int(z["n_resample"]) == 0                     # the reference never took its empty-slot resample branch
    assert len(z["losses"]) > 10 and int(z["n_greedy"]) > 10
    S, A, EP, MS, B, TF, CAP = (int(v) for v in z["meta"][:7])
    n = int(z["n_entries"])
    assert z["tree"].shape == (2 * CAP - 1,) and z["buf/states"].shape == (n, S) and len(z["actions"]) >= n
    assert int(z["frame_count"]) == len(z["losses"])     # one sample per learn step


# -- rejected arguments ------------------------------------------------------------------------------------------------
P = C.c_void_p(0x1000)                                    # stands for a valid pointer: rejected calls never follow it


def _store(capacity, **null):
    ptrs = {k: None if null.get(k) else P for k in ("states", "next_states", "actions", "rewards", "dones")}
    return N.QnetMirror(ptrs["states"], ptrs["next_states"], ptrs["actions"], ptrs["rewards"], ptrs["dones"], capacity)


def _rejected(rc, match):
    assert rc != 0
    msg = N.lib().porl_last_error().decode()
    assert match in msg, msg
    with pytest.raises(N.NativeError, match=match):
        N.check(rc, "call")


def test_per_record_rejects_bad_arguments():
    lib = N.lib()
    x = np.zeros(481, dtype=np.float32)
    xp = x.ctypes.data

    def call(tree=P, capacity=8, slot=0, state=xp, next_state=xp, S=4, store=None):
        store = _store(8) if store is None else store
        return lib.porl_per_record(tree, capacity, slot, 1.0, 1e-5, 0.6, state, next_state, S, 0, 0.0, 0.0, C.byref(store), None)
    _rejected(call(tree=None), "null")
    _rejected(call(state=None), "null")
    _rejected(call(next_state=None), "null")
    for k in ("states", "next_states", "actions", "rewards", "dones"):
        _rejected(call(store=_store(8, **{k: True})), "null")
    _rejected(lib.porl_per_record(P, 8, 0, 1.0, 1e-5, 0.6, xp, xp, 4, 0, 0.0, 0.0, None, None), "null")
    _rejected(call(capacity=0, store=_store(0)), "capacity")
    _rejected(call(capacity=8, store=_store(9)), "capacity")
    _rejected(call(S=0), "state_dim")
    _rejected(call(S=481), "too wide")
    _rejected(call(slot=-1), "slot")
    _rejected(call(slot=8), "slot")


def test_per_sample_slots_rejects_bad_arguments():
    lib = N.lib()

    def call(tree=P, capacity=8, u=P, batch=4, n_entries=8, idx=P, slots=P, w=P, wmean=P, scratch=P):
        return lib.porl_per_sample_slots(tree, capacity, u, batch, n_entries, 0.4, idx, slots, w, wmean, scratch, None)
    for k in ("tree", "u", "idx", "slots", "w", "wmean", "scratch"):
        _rejected(call(**{k: None}), "null")
    _rejected(call(capacity=0, n_entries=0), "capacity")
    _rejected(call(batch=0), "batch")
    _rejected(call(n_entries=0), "n_entries")
    _rejected(call(n_entries=9), "n_entries")


def test_per_update_f32_rejects_bad_arguments():
    lib = N.lib()

    def call(tree=P, capacity=8, idx=P, td=P, n=4, stamp=P):
        return lib.porl_per_update_f32(tree, capacity, idx, td, n, 1e-5, 0.6, stamp, None)
    for k in ("tree", "idx", "td", "stamp"):
        _rejected(call(**{k: None}), "null")
    _rejected(call(capacity=0), "capacity")
    _rejected(call(n=0), "n >= 1")
    _rejected(call(n=-3), "n >= 1")
