"""CPU-side checks of the distributional trainers' online path: the golden run of the reference's QRDQNTrainer under
train_online (scripts/gen_golden_online_dist.py) stayed clear of every greedy tie, carries the keys of the C51 online
fixture and is no larger than the PER one; porl_qnet_dist_learn turns a null and an unbound engine down before anything
is launched (so no GPU is needed to see it); and the trainers declare which learn_on their one-call step reproduces."""
import ctypes as C
import os

import pytest
import torch

from conftest import GOLDEN, load_golden
from porl_amd import _native as N


def test_golden_run_is_well_separated():
    z, _ = load_golden("online_qrdqn_s8_a4")
    c51, _ = load_golden("online_c51_s8_a4")
    top = lambda f: {k.split("/")[0] + "/" if k.split("/")[0] in ("init", "final", "final_target") else k for k in f.files}
    assert top(c51) <= top(z)                            # (parameter names differ between the two network classes)
    assert float(z["min_gap"]) >= 1e-3                   # no greedy choice near a tie: exact action equality is meaningful
    assert len(z["losses"]) > 10 and int(z["n_greedy"]) > 10
    S, A, EP, MS, THR, B, TF, CAP, seed_env, seed_np, NQ = (int(v) for v in z["meta"])
    assert (S, A, NQ, B) == (8, 4, 12, 16) and [int(h) for h in z["hidden"]] == [48, 40] and float(z["kappa"]) == 0.6
    n = len(z["actions"])
    assert n < CAP and int(z["buf/position"]) == n and z["buf/states"].shape == (n, S)      # the ring is not wrapped
    assert len(z["losses"]) == n - THR + 1               # one learn step per environment step from the threshold on
    assert os.path.getsize(os.path.join(GOLDEN, "online_qrdqn_s8_a4.npz")) <= \
        os.path.getsize(os.path.join(GOLDEN, "online_per_s8_a4.npz"))


# -- rejected arguments ------------------------------------------------------------------------------------------------
P = C.c_void_p(0x1000)                                    # stands for a valid pointer: rejected calls never follow it


def _rejected(rc, match):
    assert rc != 0
    msg = N.lib().porl_last_error().decode()
    assert match in msg, msg
    with pytest.raises(N.NativeError, match=match):
        N.check(rc, "call")


def test_dist_learn_rejects_a_null_and_an_unbound_engine():
    from porl_amd.train.cql_trainer import QnetEngine
    lib = N.lib()
    hp = N.QnetHyper(0.99, 0.0, 1.0 / 4, 1, 5e-4, 0.9, 0.999, 1e-8)
    head = N.DistHead(0, 4, 12, 1.0, 0.0, 0.0, None)

    def call(h):
        return lib.porl_qnet_dist_learn(h, P, 8, P, P, P, 8, P, P, 4, C.byref(hp), C.byref(head), None)
    _rejected(call(None), "null engine")
    eng = QnetEngine(8, 48, [16], 4, "cpu")               # created, never bound
    _rejected(call(eng._h), "porl_qnet_bind")
    # the engine's own methods refuse a CPU engine in _ensure_bound, before they look at any argument
    for method, args in ((eng.dist_learn, (hp, None, None, None, None, None, torch.zeros(4, dtype=torch.int64), head)),
                         (eng.forward_loaded, (0, 0, True, None)), (eng.backward, (None,))):
        with pytest.raises(N.NativeError, match="no CPU path"):
            method(*args)


def test_trainers_name_the_learn_on_their_one_call_step_reproduces():
    from porl_amd.train.c51_trainer import C51Trainer
    from porl_amd.train.dist_trainer import DistTrainerBase
    from porl_amd.train.qr_dqn_trainer import QRDQNTrainer
    assert DistTrainerBase._rows_for is None
    for cls in (QRDQNTrainer, C51Trainer):
        assert cls._rows_for is cls.learn_on and cls.learn is DistTrainerBase.learn

        class Mine(cls):
            def learn_on(self, *batch):
                return 0.0
        assert Mine._rows_for is not Mine.learn_on         # overriding learn_on opts out of the one-call step
    assert C.sizeof(N.DistHead) == 32 and N.ABI_VERSION == 12
