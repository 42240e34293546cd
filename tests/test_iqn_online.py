"""CPU-side checks of the IQN online path: porl_iqn_learn / porl_iqn_act turn a null and a created-but-unbound engine down
before anything is launched (so no GPU is needed to see it), porl_iqn_create enforces the engine's limits, the engine's
layout is _FlatAdam's, and the greedy-action cases of tests/test_iqn_online_gpu.py are well separated in the fp64 oracle
alone (at most 10 % of the states within 1e-4 of a tie)."""
import ctypes as C

import numpy as np
import pytest

from helpers import iqn_cases as IC
from porl_amd import _native as N

P = C.c_void_p(0x1000)                                    # stands for a valid pointer: rejected calls never follow it


def _rejected(rc, match):
    assert rc != 0
    msg = N.lib().porl_last_error().decode()
    assert match in msg, msg
    with pytest.raises(N.NativeError, match=match):
        N.check(rc, "call")


def test_learn_and_act_reject_a_null_and_an_unbound_engine():
    from porl_amd.engine import IqnEngine
    lib = N.lib()
    hp = N.IqnHyper(0.99, 1.0, 10.0, 1, 5e-4, 0.9, 0.999, 1e-8)
    src = N.QnetActSrc(1, P, 8, 0, 4, None)

    def learn(h):
        return lib.porl_iqn_learn(h, P, 8, P, P, P, 8, P, P, 4, P, 8, P, 8, C.byref(hp), None)

    def act(h):
        return lib.porl_iqn_act(h, 0, C.byref(src), P, 8, 0, P, None)
    for call in (learn, act):
        _rejected(call(None), "null engine")
    eng = IqnEngine(8, 4, 16, 32, 4, 8, "cpu")            # created, never bound
    for call in (learn, act):
        _rejected(call(eng._h), "porl_iqn_bind")
    with pytest.raises(N.NativeError, match="no CPU path"):
        eng.bind(*[None] * 5)


def test_create_enforces_the_engine_limits():
    from porl_amd.engine import IqnEngine
    IqnEngine(8, 64, 128, 32, 4, 256, "cpu")
    for kw, match in ((dict(embedding_dim=129), "embedding_dim"), (dict(max_tau=257), "max_tau"),
                      (dict(n_actions=65), "n_actions"), (dict(hidden=0), "positive")):
        args = dict(state_dim=8, n_actions=4, embedding_dim=16, hidden=32, max_batch=4, max_tau=8, device="cpu")
        args.update(kw)
        with pytest.raises(N.NativeError, match=match):
            IqnEngine(**args)
    # a layout whose tensors overlap or leave the 16-byte grid is refused
    lib = N.lib()
    eng = IqnEngine(8, 4, 16, 32, 4, 8, "cpu")
    for i, delta in ((3, -4), (5, 1)):
        offs = list(eng.offsets)
        offs[i] += delta
        cfg = N.IqnCfg(8, 4, 16, 32, 4, 8, (C.c_int64 * 10)(*offs), eng.n_params)
        h = C.c_void_p()
        _rejected(lib.porl_iqn_create(C.byref(cfg), C.byref(h)), "tensor %d" % i)
    assert C.sizeof(N.IqnHyper) == 48 and C.sizeof(N.IqnCfg) == 112 and C.sizeof(N.IqnMixProb) == 80


def test_engine_layout_is_the_flat_optimizer_layout():
    """parameters() order, every tensor on a 16-byte boundary: what _FlatAdam builds for an IQNNetwork."""
    from porl_amd.engine import IqnEngine
    from porl_amd.net.iqn_network import IQNNetwork
    for S, A, Ed, H in ((9, 5, 10, 30), (13, 3, 64, 512), (1, 1, 1, 1)):
        eng = IqnEngine(S, A, Ed, H, 4, 8, "cpu")
        off, want = 0, []
        for p in IQNNetwork(S, A, Ed, H).parameters():
            want.append(off)
            off += (p.numel() + 3) // 4 * 4
        assert eng.offsets == want and eng.n_params == off


@pytest.mark.parametrize("H,n_policy", IC.ACT_CASES)
def test_act_cases_are_well_separated_in_the_oracle(H, n_policy):
    _, states, taus, want, keep = IC.act_case(H, n_policy)
    assert states.shape == (IC.ACT_STATES, IC.ACT_S) and taus.shape == (IC.ACT_STATES, n_policy)
    assert keep.sum() >= 0.9 * IC.ACT_STATES               # at most 10 % of the states sit within 1e-4 of a tie
    assert len(set(want.tolist())) > 1                     # and the answer is not one action throughout
