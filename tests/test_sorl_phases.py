"""Two-phase SORL training (reference sorl_train_v0.py:57-103: value epochs of `vf_update`, then policy epochs of
`policy_update` with the value nets frozen) on the CPU: the numpy oracle, composed as the policy-only step composes its
work, reproduces the goldens recorded from the reference itself (scripts/gen_golden_sorl_phases.py), and the public
surface of the feature is in place."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden, sub
from oracle.por_oracle import cosine_lr, sorl_oracle, twin_forward
from porl_amd.util.synth import make_rows, split_rows
from test_oracle_golden import LOSS_RTOL, _assert_params

GOLDENS = ["sorl_2phase_s60_h64_b32", "sorl_2phase_s60_h64_b32_ln"]


def oracle_policy_update(o, obs, actions, rew, next_obs, term):
    """SORL.policy_update out of the oracle's existing pieces: twin_forward(v_tgt, s') -> TD target (sorl.py:85-89) ->
    PorOracle.policy_update(obs, target_v, actions) (sorl.py:160-176).  The value nets, the target nets and the value
    Adam state are not touched."""
    import oracle.por_oracle as O
    F = O.F32
    obs, next_obs = np.ascontiguousarray(obs, F), np.ascontiguousarray(next_obs, F)
    rew, term = np.asarray(rew, F), np.asarray(term, F)
    t1, t2, _, _ = twin_forward(o.P, o.vt, next_obs, o.L, o.layer_norm)
    target_v = (rew + (F(1.0) - term) * F(o.discount) * np.minimum(t1, t2)).astype(F)
    return o.policy_update(obs, target_v, np.ascontiguousarray(actions, F))


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_composition_reproduces_the_reference_two_phase_golden(name):
    z, meta = load_golden(name)
    S, H, L, B, KV, KP, A = (int(meta[k]) for k in ("S", "H", "L", "B", "KV", "KP", "A"))
    o = sorl_oracle(sub(z, "init/"), S, H, L, bool(meta["layer_norm"]), tau=meta["tau"], alpha=meta["alpha"],
                    max_steps=int(meta["max_steps"]))
    rows = make_rows((KV + KP) * B, S, A, seed=int(meta["seed_data"]))
    vl, gl = [], []
    for k in range(KV):
        s, r, sp, d, a = split_rows(rows[k * B:(k + 1) * B], S, A)
        vl.append(o.sorl_vf_update(s, a, r, sp, d))
    np.testing.assert_allclose(vl, z["v_loss"], rtol=LOSS_RTOL)
    _assert_params(o.P, sub(z, "mid/"))
    frozen = {k: v.copy() for k, v in o.P.items() if not k.startswith("policy.")}
    for k in range(KV, KV + KP):
        s, r, sp, d, a = split_rows(rows[k * B:(k + 1) * B], S, A)
        gl.append(oracle_policy_update(o, s, a, r, sp, d))
    np.testing.assert_allclose(gl, z["g_loss"], rtol=LOSS_RTOL)
    _assert_params(o.P, sub(z, "final/"))
    for k, v in frozen.items():                                   # value and target nets: bit-unchanged by phase two
        np.testing.assert_array_equal(o.P[k], v, err_msg=k)
    mid, final = sub(z, "mid/"), sub(z, "final/")
    for k in frozen:                                              # ... in the reference's own record as well
        np.testing.assert_array_equal(final[k], mid[k], err_msg=k)
    av, ag = sub(z, "adam_v/"), sub(z, "adam_g/")
    assert int(av["__step__"]) == KV == o.adam_v.step and int(ag["__step__"]) == KP == o.adam_g.step
    for n in o.pol_names:
        np.testing.assert_allclose(o.adam_g.m[n], ag[n + ".exp_avg"], atol=1e-6, rtol=1e-4)
    np.testing.assert_allclose(cosine_lr(meta["policy_lr"], KP, int(meta["max_steps"])), z["last_lr"][0], rtol=1e-12)


def test_policy_update_has_the_reference_signature():
    """reference agent/sorl.py:154: policy_update(agent, observations, actions, rewards, next_observations, terminals)."""
    from porl_amd.agent.sorl import SORL
    assert list(inspect.signature(SORL.policy_update).parameters) == [
        "agent", "observations", "actions", "rewards", "next_observations", "terminals"]
    assert list(inspect.signature(SORL.policy_update_from_replay).parameters) == ["agent", "replay", "batch_size"]
    assert list(inspect.signature(SORL.vf_update_from_replay).parameters) == ["agent", "replay", "batch_size"]


def test_policy_only_step_is_declared_and_bound():
    from porl_amd import _native as N
    from porl_amd.engine import IqlEngine
    header = open(os.path.join(REPO, "include", "porl_hip.h")).read()
    for sym in ("porl_iql_policy_only_step", "porl_iql_policy_only_forward"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(\s*porl_iql\s*\*\s*h\s*,\s*const\s+porl_iql_hyper\s*\*\s*hp\s*,\s*void\s*\*\s*stream\s*\)\s*;",
                         header), sym
        assert sym in N.SYMBOLS
    assert callable(IqlEngine.policy_only) and callable(IqlEngine.policy_only_forward)
