"""SORL.policy_update — the policy phase of two-phase SORL training (reference sorl_train_v0.py:57-103, agent/sorl.py:
154-176 with the TD target of sorl.py:85-89) — on the device: against the golden recorded from the reference itself,
against the fp64 oracle, and through the properties the step promises (value nets frozen, replay form equals tensor
form, joins a pipelined update, backbone, rejected calls, forced one-rank exchange).  GPU only.

Tolerances are the neighbouring tests' (tests/test_por_gpu.py): losses rtol 1e-5 (2e-5 for g_loss against the reference
golden, as test_sorl_matches_reference_golden), parameters max-abs 1e-5, against fp64 the `_cmp_params_robust` rule."""
import json
import os
import socket
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, sub
from oracle.por_oracle import PorOracle, sorl_oracle, twin_forward
from porl_amd.util.synth import make_rows, split_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LOSS_RTOL, PARAM_ATOL = 1e-5, 1e-5


def _args(S, H, L, ln=False, A=2, B=1024):
    return SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=L, layer_norm=ln, feature_dim=256,
                           action_size=A, max_batch=B)


def _np_sd(agent):
    return {k: v.detach().cpu().numpy() for k, v in agent.state_dict().items()}


def _cmp_params(got, ref, atol=PARAM_ATOL):
    worst = ("", 0.0)
    for k in ref:
        err = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
        if err > worst[1]:
            worst = (k, err)
    assert worst[1] <= atol, f"max-abs param error {worst[1]:.3e} at {worst[0]}"


def _cmp_params_robust(got, truth, frac_tol=1e-3, elem_tol=2e-6, max_tol=PARAM_ATOL):
    """tests/test_por_gpu.py:_cmp_params_robust — all but a 1e-3 share of every tensor within 2e-6 of the fp64 result,
    nothing further than 1e-5 (fp32 rounding can flip single ReLU mask bits; see there)."""
    for k, ref in truth.items():
        err = np.abs(got[k].astype(np.float64) - ref)
        frac = float((err > elem_tol).mean())
        print(f"{k}: share beyond {elem_tol:g} = {frac:.2e}, max-abs {err.max():.3e}")
        assert frac <= frac_tol, f"{k}: {frac:.2e} of elements differ by more than {elem_tol}"
        assert float(err.max()) <= max_tol, f"{k}: max-abs {err.max():.3e}"


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    import oracle.por_oracle as O
    O.set_precision(np.float32)


def _make_sorl(S, H, L, B, A=2, seed=0, ln=False, alpha=3.0, tau=0.9, max_steps=1000, **kw):
    from porl_amd.agent.sorl import SORL
    torch.manual_seed(seed)
    return SORL(_args(S, H, L, ln=ln, A=A, B=B), max_steps, tau, alpha, device=DEV, **kw)


def _batches(S, A, B, K, seed=2):
    rows = torch.from_numpy(make_rows(K * B, S, A, seed=seed)).to(DEV)
    return [split_rows(rows[k * B:(k + 1) * B], S, A) for k in range(K)]          # (s, r, s', d, a) each


def _value_state(agent):
    """Everything the policy-only step must leave alone, cloned."""
    agent.flush()
    eng = agent._engine
    return dict(params_vf=eng.params_vf.clone(), params_tgt=eng.params_tgt.clone(), adam_m_vf=eng.adam_m_vf.clone(),
                adam_v_vf=eng.adam_v_vf.clone(), stats0=eng.stats[:1].clone(), step=agent.v_optimizer.step_count)


def _assert_value_state_unchanged(agent, before):
    now = _value_state(agent)
    for k, v in before.items():
        if k == "step":
            assert now[k] == v
        else:
            assert torch.equal(now[k], v), k


def _assert_agents_equal(a, b):
    for (k, x), y in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(x, y), k
    for oa, ob in ((a.v_optimizer, b.v_optimizer), (a.policy_optimizer, b.policy_optimizer)):
        sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
        assert oa.step_count == ob.step_count and sorted(sa) == sorted(sb)
        for i in sa:
            assert torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"])
    assert a.lr_schedule.state_dict() == b.lr_schedule.state_dict()
    assert a.lr_schedule.get_last_lr() == b.lr_schedule.get_last_lr()


# ---- 3, 4: the reference's own two-phase run ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sorl_2phase_s60_h64_b32", "sorl_2phase_s60_h64_b32_ln"])
def test_two_phase_training_matches_reference_golden(name):
    z, meta = load_golden(name)
    S, H, L, B, KV, KP, A = (int(meta[k]) for k in ("S", "H", "L", "B", "KV", "KP", "A"))
    agent = _make_sorl(S, H, L, B, A=A, seed=int(meta["seed_model"]), ln=bool(meta["layer_norm"]), alpha=meta["alpha"],
                       tau=meta["tau"], max_steps=int(meta["max_steps"]))
    _cmp_params(_np_sd(agent), sub(z, "init/"), atol=0.0)
    data = _batches(S, A, B, KV + KP, seed=int(meta["seed_data"]))
    for k in range(KV):
        s, r, sp, d, a = data[k]
        np.testing.assert_allclose(agent.vf_update(s, a, r, sp, d), z["v_loss"][k], rtol=LOSS_RTOL)
    _cmp_params(_np_sd(agent), sub(z, "mid/"))
    frozen = _value_state(agent)
    for k in range(KV, KV + KP):
        s, r, sp, d, a = data[k]
        gl = agent.policy_update(s, a, r, sp, d)
        assert isinstance(gl, float)
        print(f"g_loss[{k - KV}] = {gl!r} (reference {float(z['g_loss'][k - KV])!r})")
        np.testing.assert_allclose(gl, z["g_loss"][k - KV], rtol=2e-5)
    _cmp_params(_np_sd(agent), sub(z, "final/"))
    # frozen means frozen: value nets, target nets, value Adam moments and step count bit-identical, stats[0] = last v_loss
    _assert_value_state_unchanged(agent, frozen)
    np.testing.assert_allclose(float(agent._engine.stats[0]), z["v_loss"][KV - 1], rtol=LOSS_RTOL)
    # policy Adam state and the cosine schedule against the reference's
    ag = sub(z, "adam_g/")
    st = agent.policy_optimizer.state_dict()["state"]
    names = [n for n, _ in agent.policy.named_parameters(prefix="policy")]
    assert agent.policy_optimizer.step_count == int(ag["__step__"]) == KP and len(st) == len(names)
    assert agent.v_optimizer.step_count == int(sub(z, "adam_v/")["__step__"]) == KV
    for i, n in enumerate(names):
        assert float(st[i]["step"]) == KP
        np.testing.assert_allclose(st[i]["exp_avg"].cpu().numpy(), ag[n + ".exp_avg"], atol=1e-6, rtol=1e-4, err_msg=n)
        np.testing.assert_allclose(st[i]["exp_avg_sq"].cpu().numpy(), ag[n + ".exp_avg_sq"], atol=1e-9, rtol=1e-4, err_msg=n)
    np.testing.assert_allclose(agent.lr_schedule.get_last_lr(), z["last_lr"], rtol=1e-12)
    assert agent.lr_schedule.last_epoch == KP


# ---- 5: fp64 oracle --------------------------------------------------------------------------------------------------
def _oracle_policy_update(o, s, a, r, sp, d):
    """sorl.py:85-89 then sorl.py:160-176 out of the oracle's pieces (tests/test_sorl_phases.py pins this composition
    against the reference golden)."""
    import oracle.por_oracle as O
    F = O.F32
    s, sp = np.ascontiguousarray(s, F), np.ascontiguousarray(sp, F)
    r, d = np.asarray(r, F), np.asarray(d, F)
    t1, t2, _, _ = twin_forward(o.P, o.vt, sp, o.L, o.layer_norm)
    target_v = (r + (F(1.0) - d) * F(o.discount) * np.minimum(t1, t2)).astype(F)
    return o.policy_update(s, target_v, np.ascontiguousarray(a if a is not None else sp, F))


@pytest.mark.parametrize("S,H,L,B,A,ln,alpha", [(256, 512, 2, 512, 2, False, 1.0), (60, 1024, 2, 1024, 2, False, 1.0),
                                                (17, 48, 3, 50, 5, False, 3.0), (60, 64, 2, 32, 2, True, 3.0)])
def test_policy_update_vs_fp64_oracle(S, H, L, B, A, ln, alpha):
    """Three policy-only steps from the state one device `vf_update` left, against the fp64 oracle seeded from that very
    state (so both sides start the policy phase identically; a value step's first Adam move is lr * sign(g), which two
    fp32 implementations flip on gradients within rounding of zero — nothing this step is about).  fp32 reference
    arithmetic alone (numpy fp32 oracle against fp64, same protocol, CPU): S=60/H=1024/B=1024 share 0, max 7.5e-7, loss
    5e-8; S=256/H=512/B=512 share 0, max 5.0e-7, loss 2e-8; S=17/H=48/L=3/B=50 share 0, max 2.1e-8; the LayerNorm case
    share 0, max 1.5e-8, loss 1e-7 — all well inside the caps applied here."""
    import oracle.por_oracle as O
    agent = _make_sorl(S, H, L, B, A=A, seed=0, ln=ln, alpha=alpha)
    data = _batches(S, A, B, 4, seed=2)
    s, r, sp, d, a = data[0]
    agent.vf_update(s, a, r, sp, d)
    O.set_precision(np.float64)
    o = sorl_oracle({k: v.astype(np.float64) for k, v in _np_sd(agent).items()}, S, H, L, ln, tau=0.9, alpha=alpha)
    frozen = _value_state(agent)
    for k in range(1, 4):
        s, r, sp, d, a = data[k]
        got = agent.policy_update(s, a, r, sp, d)
        want = _oracle_policy_update(o, *(t.cpu().numpy() for t in (s, a, r, sp, d)))
        print(f"step {k}: g_loss {got!r} vs fp64 {want!r} (rel {abs(got / want - 1):.2e})")
        np.testing.assert_allclose(got, want, rtol=LOSS_RTOL)
        np.testing.assert_allclose(agent.last_min_nll, o.last_min_nlp, rtol=LOSS_RTOL)
    _cmp_params_robust(_np_sd(agent), o.P)
    _assert_value_state_unchanged(agent, frozen)


def test_policy_only_step_with_the_divided_weight_formula_vs_fp64_oracle():
    """weight_mode 0 (POR's min(exp(adv / alpha), 100), policy regressing s') through the same engine entry: the second
    formula of policy_weight_kernel.  The reference has no policy-only POR step, so this goes through the agent base's
    `_policy_update`, not through a public POR method."""
    import oracle.por_oracle as O
    from porl_amd.agent.por import POR
    S, H, L, B = 20, 64, 2, 48
    torch.manual_seed(0)
    agent = POR(_args(S, H, L, B=B), 1000, 0.9, 2.0, device=DEV)
    assert agent._engine.cfg.weight_mode == 0
    data = _batches(S, 2, B, 3, seed=2)
    s, r, sp, d, _ = data[0]
    agent.por_residual_update(s, sp, r, d)              # value nets and targets differ, moments are non-zero
    sd = _np_sd(agent)
    O.set_precision(np.float64)
    o = PorOracle({k: v.astype(np.float64) for k, v in sd.items()}, S, H, L, tau=0.9, alpha=2.0)
    st = agent.goal_policy_optimizer.state_dict()["state"]
    for i, n in enumerate(o.pol_names):
        o.adam_g.m[n] = st[i]["exp_avg"].cpu().numpy().astype(np.float64)
        o.adam_g.v[n] = st[i]["exp_avg_sq"].cpu().numpy().astype(np.float64)
    o.adam_g.step, o.sched_t = 1, 1
    frozen = _value_state(agent)
    for k in range(1, 3):
        s, r, sp, d, _ = data[k]
        agent._policy_update(s, sp, r, d, sp, agent.goal_policy_optimizer, agent.goal_lr_schedule)
        got = agent._policy_loss()
        want = _oracle_policy_update(o, *(t.cpu().numpy() for t in (s, sp, r, sp, d)))
        np.testing.assert_allclose(got, want, rtol=LOSS_RTOL)
    _cmp_params_robust(_np_sd(agent), o.P)
    _assert_value_state_unchanged(agent, frozen)


# ---- 6: rows drawn on the device ---------------------------------------------------------------------------------------
def test_phase_updates_from_replay_equal_the_same_calls_on_the_drawn_rows():
    from porl_amd.buffer.replay_buffer import PackedReplay
    S, A, B, N = 60, 2, 128, 5000
    rows = make_rows(N, S, A, seed=11)
    a1, a2 = _make_sorl(S, 64, 2, B), _make_sorl(S, 64, 2, B)
    rp = PackedReplay(rows, S, A, DEV, seed=3)
    for step in range(5):
        idx = torch.empty(B, dtype=torch.int64, device=DEV)
        a1._engine.load_batch_sampled(rp.rows, B, rp.seed, rp.draws, A, True, idx_out=idx)     # peek at the draw
        draws = rp.draws
        value_phase = step < 2
        got = a1.vf_update_from_replay(rp, B) if value_phase else a1.policy_update_from_replay(rp, B)
        assert rp.draws == draws + 1
        ih = idx.cpu().numpy()
        assert len(set(ih.tolist())) == B and ih.min() >= 0 and ih.max() < N
        s, r, sp, d, a = split_rows(torch.from_numpy(rows[ih]).to(DEV), S, A)
        want = a2.vf_update(s, a, r, sp, d) if value_phase else a2.policy_update(s, a, r, sp, d)
        assert isinstance(got, float) and got == want
    _assert_agents_equal(a1, a2)
    assert a1.v_optimizer.step_count == 2 and a1.policy_optimizer.step_count == 3


# ---- 7: between pipelined updates --------------------------------------------------------------------------------------
@pytest.fixture(params=[0, 7], ids=["gemm-path", "skinny-path"])
def same_kernels_in_both_modes(request):
    """tests/test_por_gpu.py:same_kernels_in_both_modes — the pipelined and the one-stream update choose the kernels of
    their <= 64-wide products separately; "pipelining only reorders" is a statement about equal kernels, so one
    selection is pinned for both (engines copy the process defaults when they are created)."""
    from porl_amd import engine as E
    E.tune_set("skinny", request.param)
    E.tune_set("skinny_pipelined", request.param)
    yield request.param
    E.tune_set("skinny", 7)
    E.tune_set("skinny_pipelined", -1)


def test_policy_update_between_pipelined_updates_equals_the_synchronous_run(same_kernels_in_both_modes):
    """A pipelined `update_from_replay` leaves its policy phase on the side stream; the policy-only step that follows
    reads and writes the same policy parameters, moments and scratch, so it must join that phase first."""
    from porl_amd.buffer.replay_buffer import PackedReplay
    S, A, B, H = 60, 2, 256, 256
    rows = make_rows(20_000, S, A, seed=5)
    extra = _batches(S, A, B, 2, seed=6)
    a_sync, a_pipe = _make_sorl(S, H, 2, B), _make_sorl(S, H, 2, B)
    a_pipe.async_losses = True
    assert a_pipe.pipeline
    hist = {id(a_sync): [], id(a_pipe): []}
    for ag in (a_sync, a_pipe):
        rp = PackedReplay(rows, S, A, DEV, seed=4)
        for k in range(3):
            ag.update_from_replay(rp, B)
        if ag is a_pipe:
            assert ag._engine._policy_done is not None          # a policy phase is outstanding on the side stream
        for s, r, sp, d, a in extra:
            out = ag.policy_update(s, a, r, sp, d)
            hist[id(ag)].append(float(out[0]) if ag.async_losses else out)
            if ag.async_losses:
                assert isinstance(out, torch.Tensor) and out.shape == (1,)
        for k in range(2):
            ag.update_from_replay(rp, B)
    _assert_agents_equal(a_pipe, a_sync)
    assert hist[id(a_pipe)] == hist[id(a_sync)]


# ---- 8: backbone -------------------------------------------------------------------------------------------------------
def test_policy_update_with_encoder_backbone_equals_heads_on_the_encoded_states():
    from porl_amd.agent.fasternet import FasterNet
    from porl_amd.agent.sorl import SORL
    z, _ = load_golden("sorl_enc_b6")                  # (B, 362) states, actions, rewards, terminals of that fixture
    B, K, H, L, A, F = (int(v) for v in z["meta"])
    torch.manual_seed(int(z["seed_model"]))
    backbone = FasterNet(3, F, max_batch=B).eval()
    args = SimpleNamespace(state_size=362, feature_dim=F, hidden_dim=H, n_hidden=L, layer_norm=False, action_size=A,
                           max_batch=B)
    with_enc = SORL(args, max_steps=50, tau=0.9, alpha=3.0, device=DEV, backbone=backbone)
    heads = SORL(SimpleNamespace(**{**vars(args), "state_size": F}), max_steps=50, tau=0.9, alpha=3.0, device=DEV)
    heads.load_state_dict({k: v for k, v in with_enc.state_dict().items() if not k.startswith("backbone.")})
    t = lambda n, k: torch.from_numpy(z[f"{n}{k}"].copy()).to(DEV)
    for ag, enc in ((with_enc, lambda x: x), (heads, with_enc.backbone)):
        ag.vf_update(enc(t("s", 0)), t("a", 0), t("r", 0), enc(t("s2", 0)), t("d", 0))
    for k in range(1, K):
        got = with_enc.policy_update(t("s", k), t("a", k), t("r", k), t("s2", k), t("d", k))
        want = heads.policy_update(with_enc.backbone(t("s", k)), t("a", k), t("r", k), with_enc.backbone(t("s2", k)), t("d", k))
        assert got == want
    sd = with_enc.state_dict()
    for k, v in heads.state_dict().items():
        assert torch.equal(sd[k], v), k
    assert with_enc.policy_optimizer.step_count == K - 1 and with_enc.v_optimizer.step_count == 1


# ---- 9: rejected calls -------------------------------------------------------------------------------------------------
def test_oversized_batch_is_rejected_without_side_effects():
    from porl_amd import _native as N
    from porl_amd.buffer.replay_buffer import PackedReplay
    S, A, B, H = 60, 2, 64, 64
    a, b = _make_sorl(S, H, 2, B), _make_sorl(S, H, 2, B)
    data = _batches(S, A, B, 3, seed=2)
    big = _batches(S, A, B + 1, 1, seed=3)[0]
    rows = make_rows(5_000, S, A, seed=9)
    ra = PackedReplay(rows, S, A, DEV, seed=4)
    for ag in (a, b):
        s, r, sp, d, act = data[0]
        ag.vf_update(s, act, r, sp, d)
        s, r, sp, d, act = data[1]
        ag.policy_update(s, act, r, sp, d)
    before = {k: v.clone() for k, v in a.state_dict().items()}
    stats = a._engine.stats.clone()
    s, r, sp, d, act = big
    with pytest.raises(RuntimeError):
        a.policy_update(s, act, r, sp, d)                     # max_batch is B
    with pytest.raises(N.NativeError):
        a.policy_update_from_replay(ra, B + 1)
    assert ra.draws == 0
    assert a.policy_optimizer.step_count == 1 and a.v_optimizer.step_count == 1
    assert a.lr_schedule.last_epoch == 1 and a.lr_schedule.get_last_lr() == b.lr_schedule.get_last_lr()
    for k, v in a.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert torch.equal(a._engine.stats, stats)
    s, r, sp, d, act = data[2]
    assert a.policy_update(s, act, r, sp, d) == b.policy_update(s, act, r, sp, d)
    _assert_agents_equal(a, b)


def test_policy_only_step_needs_a_bound_engine_and_a_loaded_batch():
    """Error conventions of porl_iql_step: an error code and porl_last_error, nothing launched."""
    import ctypes as C
    from porl_amd import _native as N
    from porl_amd.engine import IqlEngine
    eng = IqlEngine(8, 2, 32, 2, pol_tanh=True, weight_mode=1, max_batch=16, device=DEV)
    hp = eng.hyper()
    for name in ("porl_iql_policy_only_step", "porl_iql_policy_only_forward"):
        rc = getattr(eng._lib, name)(eng._h, C.byref(hp), N.current_stream_ptr(DEV))
        assert rc != 0 and b"bind" in eng._lib.porl_last_error()
    eng._ensure_bound()
    for fn in (eng.policy_only, eng.policy_only_forward):
        with pytest.raises(N.NativeError, match="no minibatch loaded"):
            fn(hp)
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    eng.load_batch(z(4, 8), z(4, 8), z(4), z(4), None)                    # a value-phase batch: no policy target
    with pytest.raises(N.NativeError, match="pol_target"):
        eng.policy_only(hp)


# ---- 10: forced one-rank exchange --------------------------------------------------------------------------------------
def test_policy_update_through_the_forced_one_rank_exchange():
    """The data-parallel branch of the policy-only step (forward half, backward, reduce-scatter + sharded Adam +
    all-gather or all-reduce + Adam, statistics all-reduce) on a one-rank RCCL group with the exchange forced on, in a
    process of its own: per update from identical state it must reproduce the plain step at the per-update bars of
    tests/test_rccl_gpu.py (gradients 1e-6 of each tensor's largest element, losses 1e-6 relative, parameters 2e-6)."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "helpers", "sorl_policy_world1.py"), str(port)],
                       env=env, capture_output=True, text=True, timeout=300)
    skip = [ln for ln in r.stdout.splitlines() if ln.startswith("SORL_POLICY_WORLD1_SKIP ")]
    if skip:
        pytest.skip(skip[0][len("SORL_POLICY_WORLD1_SKIP "):])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("SORL_POLICY_WORLD1 ")]
    assert len(line) == 1
    out = json.loads(line[0][len("SORL_POLICY_WORLD1 "):])
    assert out["backend"] == "nccl" and out["world"] == 1
    assert [c["exchange"] for c in out["cases"]] == ["reduce_scatter", "all_reduce"]
    for c in out["cases"]:
        assert len(c["per_update"]) == 3 and c["value_state_unchanged"] is True, c
        for u in c["per_update"]:
            assert u["max_rel_grad_err"] <= 1e-6 and u["max_rel_loss_err"] <= 1e-6 and u["max_abs_param_err"] <= 2e-6, c
