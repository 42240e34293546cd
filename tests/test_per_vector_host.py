"""CPU-side checks of prioritized replay for the vectorised loop (csrc/per_vector.hpp): porl_per_fill_range and
porl_per_sample_keyed turn bad arguments down before anything is launched (through ctypes with a null stream and sentinel
buffers, and in a stand-alone program under the host sanitizers), the keyed uniforms of tests/helpers/per_vector_cases.py lie
in [0, 1) and keep apart from the simulator's stream under the same seed, and the helper's brute-force node set equals the
range rule the kernel walks by."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import navsim_cases as NC
from helpers import per_vector_cases as PV
from porl_amd import _native as N

INF, NAN = float("inf"), float("nan")


def _rejected(rc, match):
    assert rc == -1, rc                                   # PORL_ERR_INVALID
    msg = N.lib().porl_last_error().decode()
    assert match in msg, msg
    with pytest.raises(N.NativeError, match=match):
        N.check(rc, "call")


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def test_fill_range_rejects_bad_arguments_before_a_launch():
    lib = N.lib()
    tree = np.full(15, 7.0)                               # host memory with a sentinel: a rejected call never follows it

    def call(tree_=tree, capacity=8, first=0, n=4, td=1.0, eps=1e-5, alpha=0.6):
        return lib.porl_per_fill_range(None if tree_ is None else _ptr(tree_), capacity, first, n, td, eps, alpha, None)
    _rejected(call(tree_=None), "null tree")
    for cap in (0, -8, 2 ** 63 - 1):
        _rejected(call(capacity=cap, n=0), "capacity")
    for n in (-1, 9, 2 ** 63 - 1):
        _rejected(call(n=n), "n ")
    for first in (-1, 8, 2 ** 63 - 1):
        _rejected(call(first=first), "first_slot")
    _rejected(call(first=8, n=0), "first_slot")
    for bad in (NAN, INF, -INF):
        _rejected(call(td=bad), "td_error")
        _rejected(call(eps=bad), "eps")
        _rejected(call(alpha=bad), "alpha")
    assert (tree == 7.0).all()


def test_fill_range_of_nothing_is_ok_without_a_launch():
    lib = N.lib()
    tree = np.full(15, 7.0)
    for cap, first in ((8, 0), (8, 7), (1, 0)):
        assert lib.porl_per_fill_range(_ptr(tree), cap, first, 0, 1.0, 1e-5, 0.6, None) == 0
    assert (tree == 7.0).all()


def test_sample_keyed_rejects_bad_arguments_before_a_launch():
    lib = N.lib()
    bufs = dict(tree=np.full(15, 7.0), idx=np.full(4, 7, np.int64), slots=np.full(4, 7, np.int64), w=np.full(4, 7, np.float32),
                wmean=np.full(1, 7, np.float32), scratch=np.full(4, 7.0))

    def call(capacity=8, draw=0, batch=4, n_entries=8, **null):
        p = {k: None if null.get(k) else _ptr(v) for k, v in bufs.items()}
        return lib.porl_per_sample_keyed(p["tree"], capacity, 5, draw, batch, n_entries, 0.4, p["idx"], p["slots"], p["w"],
                                         p["wmean"], p["scratch"], None)
    for k in bufs:
        _rejected(call(**{k: True}), "null")
    _rejected(call(capacity=0, n_entries=0), "capacity")
    _rejected(call(batch=0), "batch")
    _rejected(call(batch=-4), "batch")
    _rejected(call(n_entries=0), "n_entries")
    _rejected(call(n_entries=9), "n_entries")
    for draw in (-1, 2 ** 32, 2 ** 63 - 1):
        _rejected(call(draw=draw), "draw")
    for v in bufs.values():
        assert (v == 7).all()


def test_rejected_arguments_under_sanitizers():
    """tests/helpers/abi_reject_per_vector.cpp on the host-only sanitized build: every rejected argument of the two entry
    points comes back as PORL_ERR_INVALID with a message that names it, before any HIP call; ASan / UBSan abort the process
    on any finding.  A stand-alone program: nothing sanitized is loaded into this interpreter."""
    from porl_amd import build as Bd
    assert Bd.build_sanitized_per_vector(verbose=False) == Bd.SAN_PER_VECTOR_DRIVER
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([Bd.SAN_PER_VECTOR_DRIVER], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "0 unexpected" in r.stdout
    assert int(r.stdout.split("abi_reject_per_vector:")[1].split("checks")[0]) >= 36


# ---- the keyed stream -----------------------------------------------------------------------------------------------------
def test_the_tag_is_no_robot_key():
    assert PV.TAG == NC.sm64(PV.TAG_SOURCE)                # sm64 is a bijection: TAG = sm64(e) only for e = TAG_SOURCE,
    assert PV.TAG_SOURCE > 2 ** 40 + 2 ** 24               # which is no robot index (env_offset <= 2^40, n <= 2^24)


def test_keyed_u_lies_in_the_unit_interval_and_moves_with_every_argument():
    us = np.array([[PV.keyed_u(seed, draw, i) for i in range(64)] for seed in (0, 5, 2 ** 64 - 1) for draw in (0, 1, 2 ** 32 - 1)])
    assert ((us >= 0.0) & (us < 1.0)).all()
    assert len(set(us.reshape(-1).tolist())) == us.size    # no two of the 576 agree: draws, positions and seeds all move it
    assert 0.4 < us.mean() < 0.6
    # the counter's two halves do not alias: (draw, i) = (0, 1) and (1, 0) are different counters
    assert PV.keyed_u(5, 0, 1) != PV.keyed_u(5, 1, 0)
    assert PV.keyed_us(5, 3, 8).tolist() == [PV.keyed_u(5, 3, i) for i in range(8)]


def test_keyed_u_is_apart_from_the_simulator_and_selection_stream():
    """Under the same seed, robot e's draws (exploration at act-step t, resets of episode t) are u01(robot_key(seed, e), t, j):
    none of a grid of them equals a keyed uniform of the same seed."""
    for seed in (0, 5):
        keyed = {PV.keyed_u(seed, d, i) for d in range(8) for i in range(64)}
        sim = {NC.u01(NC.robot_key(seed, e), t, j) for e in range(64) for t in range(8) for j in range(2)}
        assert len(keyed) == 512 and not keyed & sim
        assert PV.keyed_key(seed) not in {NC.robot_key(seed, e) for e in range(4096)}


# ---- the node set of a fill -----------------------------------------------------------------------------------------------
def test_range_nodes_is_the_range_recursion():
    """Brute-force leaf-to-root walks == runs of tree indices halved toward the root, for every (capacity, first_slot, n)
    with capacity 1..40 — wrapped rings and both leaf depths included."""
    cases = 0
    for cap in range(1, 41):
        for first in range(cap):
            for n in range(cap + 1):
                assert PV.range_nodes(cap, first, n) == PV.range_recursion(cap, first, n), (cap, first, n)
                cases += 1
    assert cases == sum(c * (c + 1) for c in range(1, 41))


def test_rebuild_sums_children():
    rng = np.random.default_rng(0)
    for cap in (1, 2, 3, 5, 8, 13):
        t = np.zeros(2 * cap - 1)
        t[cap - 1:] = rng.uniform(0.1, 2.0, cap)
        r = PV.rebuild(t, cap)
        assert (r[cap - 1:] == t[cap - 1:]).all() and abs(r[0] - t[cap - 1:].sum()) <= 1e-12 * cap
        for p in range(cap - 1):
            assert r[p] == r[2 * p + 1] + r[2 * p + 2]
