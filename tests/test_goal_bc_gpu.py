"""Goal-conditioned behaviour cloning on the device (porl_amd.agent.goal_bc.GoalConditionedBC over porl_iql_load_batch_cat /
porl_iql_load_batch_pairs / porl_iql_bc_forward / porl_iql_bc_step; reference agent/por.py:178-184): against the golden
recorded from the reference's unmodified method, per element against the fp64 restatement of tests/helpers/bc_cases.py,
the staging kernel bit for bit against the existing gather paths, what the step must leave alone, the rejected calls, and
POR acting through the trained policy.  GPU only.

Tolerances: against the golden the bounds of tests/test_sorl_phases_gpu.py (losses rtol 2e-5, parameters and moments
max-abs 1e-5, seeded initialisation bit-equal); per element max(2e-6, 4 x e32) with e32 the error of the numpy fp32 run
(forward_cases' constants and rule), error = max |got - ref64| / max |ref64| per tensor; parameters after one step by the
`_cmp_params_robust` rule; staging comparisons have no tolerance.

Measured on an MI355X, the output closest to its bar per configuration (over its batches and both store layouts, which
give the same bits):
  s60_g60_c61_a2_h48_l2       policy.net.2.weight  e32 5.89e-07  kernel 8.50e-07  bar 2.35e-06  (B = 1030)
  s60_g2_c0_a2_h132_l2_tanh   policy.net.4.weight  e32 4.84e-07  kernel 9.21e-07  bar 2.00e-06  (B = 65)
  s3_g1_c4_a1_h30_l1_tanh     policy.net.0.weight  e32 1.92e-07  kernel 2.93e-07  bar 2.00e-06  (B = 130)
  s17_g17_c0_a6_h48_l3        policy.net.4.bias    e32 1.56e-06  kernel 2.48e-06  bar 6.23e-06  (B = 130)
  s182_g182_c183_a2_h48_l2    stats1               e32 2.38e-07  kernel 9.60e-07  bar 2.00e-06  (B = 1)
Parameters after one step stay within 1.4e-7 of the fp64 step everywhere.  The 53 cases take 5 s."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from helpers import bc_cases as BCC
from oracle import por_oracle as O
from porl_amd import _native as N
from porl_amd import engine as E
from porl_amd.engine import IqlEngine
from porl_amd.util.synth import make_rows, split_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LOSS_RTOL, PARAM_ATOL = 2e-5, 1e-5
SENTINEL = 1.0e4


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    O.set_precision(np.float32)


def _make_bc(S, G, A, H=64, L=2, B=128, seed=0, **kw):
    from porl_amd.agent import GoalConditionedBC
    torch.manual_seed(seed)
    return GoalConditionedBC(S, G, A, kw.pop("max_steps", 1000), hidden_dim=H, n_hidden=L, device=DEV, max_batch=B, **kw)


def _np_sd(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


def _assert_same(a, b):
    """Two trainers hold the same bits: parameters, Adam moments and step count, schedule."""
    for (k, x), y in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(x, y), k
    sa, sb = a.policy_optimizer.state_dict()["state"], b.policy_optimizer.state_dict()["state"]
    assert a.policy_optimizer.step_count == b.policy_optimizer.step_count and sorted(sa) == sorted(sb)
    for i in sa:
        assert torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"])
    assert a.policy_lr_schedule.state_dict() == b.policy_lr_schedule.state_dict()


def _cmp_params_robust(got, truth, frac_tol=1e-3, elem_tol=2e-6, max_tol=PARAM_ATOL):
    """tests/test_por_gpu.py:_cmp_params_robust — all but a 1e-3 share of every tensor within 2e-6 of the fp64 result,
    nothing further than 1e-5."""
    for k, ref in truth.items():
        err = np.abs(got[k].astype(np.float64) - ref)
        frac = float((err > elem_tol).mean())
        print(f"{k}: share beyond {elem_tol:g} = {frac:.2e}, max-abs {err.max():.3e}")
        assert frac <= frac_tol, f"{k}: {frac:.2e} of elements differ by more than {elem_tol}"
        assert float(err.max()) <= max_tol, f"{k}: max-abs {err.max():.3e}"


# ---- 1: the reference's own run ------------------------------------------------------------------------------------------
def test_five_updates_reproduce_the_reference_golden():
    z, meta = load_golden("goal_bc_s60_h64_b32")
    S, G, H, L, B, K, A = (int(meta[k]) for k in ("S", "G", "H", "L", "B", "K", "A"))
    bc = _make_bc(S, G, A, H, L, B, seed=int(meta["seed_model"]), max_steps=int(meta["max_steps"]), policy_lr=meta["policy_lr"])
    init = sub(z, "init/")
    assert list(bc.state_dict().keys()) == list(init.keys())
    for k, v in _np_sd(bc).items():
        assert np.array_equal(v, init[k]), k                                   # seeded initialisation: bit-equal
    rows = torch.from_numpy(make_rows(K * B, S, A, seed=int(meta["seed_data"]))).to(DEV)
    for k in range(K):
        s, _, sp, _, a = split_rows(rows[k * B:(k + 1) * B], S, A)             # strided views of the packed rows: no cat
        loss = bc.update(s, sp, a)
        assert isinstance(loss, float)
        print(f"policy_loss[{k}] = {loss!r} (reference {float(z['policy_loss'][k])!r})")
        np.testing.assert_allclose(loss, z["policy_loss"][k], rtol=LOSS_RTOL)
    final, adam = sub(z, "final/"), sub(z, "adam/")
    got = _np_sd(bc)
    st = bc.policy_optimizer.state_dict()["state"]
    names = [n for n, _ in bc.policy.named_parameters(prefix="policy")]
    assert names == list(final.keys()) and len(st) == len(names)
    assert bc.policy_optimizer.step_count == int(adam["__step__"]) == K
    for i, n in enumerate(names):
        assert float(np.abs(got[n].astype(np.float64) - final[n]).max()) <= PARAM_ATOL, n
        assert float(st[i]["step"]) == K
        for part in ("exp_avg", "exp_avg_sq"):
            err = float(np.abs(st[i][part].cpu().numpy().astype(np.float64) - adam[f"{n}.{part}"]).max())
            assert err <= PARAM_ATOL, (n, part, err)
    np.testing.assert_allclose(bc.policy_lr_schedule.get_last_lr(), z["last_lr"], rtol=1e-12)
    assert bc.policy_lr_schedule.last_epoch == K and bc.last_min_nll is not None


# ---- 2: per element against fp64 -----------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def shared_engine(name):
    cfg, _ = BCC.params(name)
    return IqlEngine(cfg.S + cfg.G, cfg.A, cfg.H, cfg.L, False, cfg.tanh, weight_mode=1, max_batch=BCC.max_batch_of(name),
                     device=DEV)


def reset_engine(name):
    """bc_cases.params in a sentinel-filled policy arena; every other arena, the statistics and the workspace hold the
    sentinel too, so that whatever the step reads without its producer having written it, or writes outside its own, shows."""
    cfg, P = BCC.params(name)
    eng = shared_engine(name)
    eng._ensure_bound()
    for k in ("params_vf", "params_tgt", "params_pol", "grads_vf", "grads_pol", "adam_m_vf", "adam_v_vf", "stats", "workspace"):
        getattr(eng, k).fill_(SENTINEL)
    eng.adam_m_pol.zero_()
    eng.adam_v_pol.zero_()
    table = eng.tensor_table(1)
    assert [shape for _, shape in table] == [P[n].shape for n in BCC.param_names(cfg)]
    for view, n in zip(IqlEngine.views(eng.params_pol, table), BCC.param_names(cfg)):
        view.copy_(torch.from_numpy(np.array(P[n])))
    eng.set_mode(0)
    return cfg, eng


@lru_cache(maxsize=None)
def store(name, layout):
    """The configuration's row store on the device.  "lanes": pitch a multiple of 4 floats on an allocation boundary, so the
    s segment moves as 16-byte lanes; "odd": an odd pitch, so no row after the first starts on 16 bytes."""
    rows = BCC.pool(name)["rows"]
    n, W = rows.shape
    pitch = (W + 3) // 4 * 4 if layout == "lanes" else (W if W % 2 else W + 1)
    buf = torch.full((n, pitch), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[:, :W]
    view.copy_(torch.from_numpy(np.array(rows)))
    assert view.stride(0) == pitch and (pitch % 4 == 0) == (layout == "lanes")
    return view


def read_grads(eng, cfg):
    return {n: v.cpu().numpy().copy() for n, v in zip(BCC.param_names(cfg), IqlEngine.views(eng.grads_pol, eng.tensor_table(1)))}


@pytest.mark.parametrize("layout", ["lanes", "odd"])
@pytest.mark.parametrize("name,B", BCC.RUNS, ids=[f"{n}-b{B}" for n, B in BCC.RUNS])
def test_gradients_and_one_step_match_the_fp64_restatement(name, B, layout):
    cfg, eng = reset_engine(name)
    ref = BCC.reference(name, B)
    rows = store(name, layout)
    start, goal = (torch.from_numpy(a).to(DEV) for a in BCC.pairs(name, B))
    frozen = {k: getattr(eng, k).clone() for k in ("params_vf", "params_tgt", "params_pol", "adam_m_vf", "adam_v_vf", "grads_vf")}

    def load():
        eng.load_batch_pairs(rows, B, cfg.S, cfg.A, cfg.goal_col, cfg.G, start=start, goal=goal)

    # -- bc_forward + policy_backward: every gradient tensor of group 1, stats[1:3] --
    hp = eng.hyper(inv_batch=1.0 / B, policy_lr=O.cosine_lr(BCC.LR0, 0, BCC.T_MAX), policy_step=1)
    load()
    eng.bc_forward(hp)
    eng.policy_backward(hp)
    got = dict(grads=read_grads(eng, cfg), stats=eng.stats[1:3].cpu().numpy().copy())
    over = []
    for k, err in BCC.errors(cfg, got, ref["ref"]).items():
        print(f"{name} b{B} {layout} {k}: error {err:.2e}  e32 {ref['e32'][k]:.2e}  bar {ref['bar'][k]:.2e}")
        if not err <= ref["bar"][k]:
            over.append((k, err, ref["bar"][k]))
    assert not over, f"over the bar: {over}"
    assert not got["grads"][BCC.PREFIX + ".log_std"][BCC.clamped_out(name)].any(), "d/dlog_std outside [-5, 2] is not exactly zero"
    for k, v in frozen.items():
        assert torch.equal(getattr(eng, k), v), f"{k} changed"
    assert float(eng.stats[0]) == SENTINEL and bool((eng.stats[3:] == SENTINEL).all())
    # -- one bc_step from the same state --
    load()
    eng.bc_step(hp)
    params = {n: v.cpu().numpy() for n, v in zip(BCC.param_names(cfg), IqlEngine.views(eng.params_pol, eng.tensor_table(1)))}
    _cmp_params_robust(params, ref["params64"])
    np.testing.assert_array_equal(eng.stats[1:3].cpu().numpy(), got["stats"])       # the step's loss is the scored one
    for k, v in frozen.items():
        if k != "params_pol":
            assert torch.equal(getattr(eng, k), v), f"{k} changed"
    assert float(eng.stats[0]) == SENTINEL


# ---- 3: staging, bit for bit ---------------------------------------------------------------------------------------------
def _replays(S, A, n=4000, seed=11, rseed=3):
    from porl_amd.buffer.replay_buffer import PackedReplay
    rows = make_rows(n, S, A, seed=seed)
    return rows, PackedReplay(rows, S, A, DEV, seed=rseed), PackedReplay(rows, S, A, DEV, seed=rseed)


@pytest.mark.parametrize("G,B", [(20, 37), (2, 64)])
def test_hindsight_update_from_replay_equals_rvs_sample_batch_then_update(G, B):
    from porl_amd.dataloader.episodes import EpisodeIndex, hindsight_indices, rvs_sample_batch
    S, A = 20, 3
    rows, r1, r2 = _replays(S, A)
    a, b = _make_bc(S, G, A), _make_bc(S, G, A)
    index = EpisodeIndex.from_replay(r1)
    for step in range(3):
        # the rows the kernel draws are hindsight_indices' for the same key, index for index
        so, go = (torch.empty(B, dtype=torch.int64, device=DEV) for _ in range(2))
        a._engine.load_batch_pairs(r1.rows, B, S, A, 0, G, episodes=index, seed=r1.seed, step=r1.draws, start_out=so, goal_out=go)
        hs, hg = hindsight_indices(index, B, seed=r1.seed, step=r1.draws)
        assert torch.equal(so, hs) and torch.equal(go, hg)
        assert bool((hg >= hs).all()) and int(hg.max()) < len(r1)
        got = a.update_from_replay(r1, B, goal="hindsight")
        batch = rvs_sample_batch(r2, B)
        want = b.update(batch["observations"], batch["next_observations"][:, :G], batch["actions"])
        assert isinstance(got, float) and got == want
        assert r1.draws == r2.draws == step + 1
    assert r1._episode_index.n_episodes == index.n_episodes                    # cached on the replay, as rvs_sample_batch does
    _assert_same(a, b)


def test_next_goal_update_from_replay_equals_sample_gather_update():
    S, A, B = 20, 3, 50
    rows, r1, r2 = _replays(S, A)
    a, b = _make_bc(S, S, A), _make_bc(S, S, A)
    for step in range(3):
        got = a.update_from_replay(r1, B)                                       # goal="next": the same row's s'
        s, _, sp, _, act = r2.split(r2.gather(r2.sample_indices(B)))
        assert got == b.update(s, sp, act)
        assert r1.draws == r2.draws == step + 1
    _assert_same(a, b)
    # evaluate moves nothing and returns what the next update on the same rows returns
    before = {k: v.clone() for k, v in a.state_dict().items()}
    draws, steps, epoch = r1.draws, a.policy_optimizer.step_count, a.policy_lr_schedule.last_epoch
    idx = r2.sample_indices(B).clone()
    s, _, sp, _, act = r2.split(r2.gather(idx))
    scored = [a.evaluate_from_replay(r1, B, indices=idx), a.evaluate(s, sp, act)]
    assert r1.draws == draws
    drawn = a.evaluate_from_replay(r1, B)
    assert r1.draws == draws + 1
    whole = a.evaluate_store(SimpleNamespace(rows=r1.rows[:130], obs_dim=S, act_dim=A), batch_size=64)
    assert whole["n_rows"] == 130 and np.isfinite(whole["loss"]) and whole["min_nll"] <= whole["loss"]
    for k, v in a.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert a.policy_optimizer.step_count == steps and a.policy_lr_schedule.last_epoch == epoch
    _assert_same(a, b)
    assert isinstance(drawn, float)
    assert scored[0] == scored[1] == a.update_from_replay(r1, B, indices=idx)
    assert r1.draws == draws + 1


def test_given_pairs_with_duplicates_equal_rows_and_the_last_row():
    S, A, G = 20, 3, 20
    rows, r1, _ = _replays(S, A)
    n = len(r1)
    start = torch.tensor([n - 1, 0, 0, 5, n - 1, 7, 3], dtype=torch.int64, device=DEV)      # B = 7: not a multiple of 4
    goal = torch.tensor([n - 1, 0, 4, 5, 2, n - 1, 3], dtype=torch.int64, device=DEV)
    a, b, c = _make_bc(S, G, A), _make_bc(S, G, A), _make_bc(S, G, A)
    got = a.update_from_replay(r1, 7, goal="hindsight", indices=start, goal_indices=goal)
    dr = r1.rows
    want = b.update(dr[start, :S], dr[goal, :S], dr[start, 2 * S + 2:])                     # dense tensors: the cat loader
    assert got == want and r1.draws == 0
    _assert_same(a, b)
    # the same pairs through POR's column: goal = s' of the goal row
    got = c.update_from_replay(r1, 7, goal="hindsight", indices=start, goal_indices=goal, goal_col=S + 1)
    d = _make_bc(S, G, A)
    assert got == d.update(dr[start, :S], dr[goal, S + 1:2 * S + 1], dr[start, 2 * S + 2:])
    _assert_same(c, d)


@pytest.mark.parametrize("bad", [-1, "n"])
def test_an_index_outside_the_store_is_a_nan_loss_and_the_store_is_untouched(bad):
    S, A = 20, 3
    rows, r1, _ = _replays(S, A, n=500)
    bc = _make_bc(S, S, A)
    before = r1.rows.clone()
    idx = torch.arange(9, dtype=torch.int64, device=DEV)
    idx[4] = len(r1) if bad == "n" else bad
    with pytest.raises(ValueError, match="NaN loss"):
        bc.update_from_replay(r1, 9, indices=idx)
    fresh = _make_bc(S, S, A)                                                   # (the first one's parameters are NaN by now)
    with pytest.raises(ValueError, match="NaN loss"):
        fresh.evaluate_from_replay(r1, 9, goal="hindsight", indices=torch.arange(9, device=DEV), goal_indices=idx)
    ok = torch.arange(9, dtype=torch.int64, device=DEV)
    assert np.isfinite(fresh.evaluate_from_replay(r1, 9, goal="hindsight", indices=ok, goal_indices=ok))
    assert torch.equal(r1.rows, before) and r1.draws == 0


# ---- 4: isolation ----------------------------------------------------------------------------------------------------------
def test_the_step_touches_the_policy_group_only_and_launches_no_value_net():
    S, G, A, H, L, B = 20, 20, 3, 64, 3, 50
    rows, r1, _ = _replays(S, A)
    bc = _make_bc(S, G, A, H, L)
    eng = bc._engine
    eng._ensure_bound()
    gen = torch.Generator(device=DEV).manual_seed(1)
    for k in ("params_vf", "params_tgt", "adam_m_vf", "adam_v_vf", "grads_vf"):
        getattr(eng, k).copy_(torch.randn(getattr(eng, k).shape, device=DEV, generator=gen))
    eng.stats.fill_(123.0)
    frozen = {k: getattr(eng, k).clone() for k in ("params_vf", "params_tgt", "adam_m_vf", "adam_v_vf", "grads_vf")}
    bc.update_from_replay(r1, B)                                                # first use: bind, warm
    E.prof_enable(True)
    try:
        bc.update_from_replay(r1, B)
        prof = {p["name"]: p["launches"] for p in E.prof_read(512) if p["launches"]}
    finally:
        E.prof_enable(False)
    print(prof)
    hidden = {k: v for k, v in prof.items() if k.startswith(("B1.", "B2."))}
    assert sum(hidden.values()) == L                                           # one net per launch, one launch per layer
    assert sum(v for k, v in prof.items() if k.startswith("B0.") and k.endswith("stage_pairs_kernel")) == 1
    assert sum(v for k, v in prof.items() if k.endswith("policy_nll_kernel")) == 1 and "B4.policy_nll_kernel" in prof
    assert sum(v for k, v in prof.items() if k.endswith("adam_ema_kernel")) == 1 and "B9.adam_ema_kernel" in prof
    for k in prof:
        assert not k.startswith(("V", "O", "P1.", "P2.", "P3.", "P4.")), k       # no value phase, no twin forward
        assert "policy_weight_kernel" not in k and "relu_head" not in k and "sampled_batch" not in k, k
    assert sum(prof.values()) == 2 * L + 4 + 1                                 # the step and its one staging launch
    for k, v in frozen.items():
        assert torch.equal(getattr(eng, k), v), k
    assert float(eng.stats[0]) == 123.0 and bool((eng.stats[3:] == 123.0).all())


# ---- 5: rejected calls -----------------------------------------------------------------------------------------------------
def test_phase_calls_refuse_a_batch_of_the_other_kind_by_name():
    S, G, A, B = 20, 20, 3, 16
    eng = IqlEngine(S + G, A, 32, 2, weight_mode=1, max_batch=B, device=DEV)
    eng._ensure_bound()
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    hp = eng.hyper(inv_batch=1.0 / B)
    eng.stats.fill_(7.0)
    eng.workspace.fill_(SENTINEL)
    eng.load_batch_cat(z(B, S), z(B, G), z(B, A))
    torch.cuda.synchronize()
    ws, pol = eng.workspace.clone(), eng.params_pol.clone()
    E.prof_enable(True)
    try:
        for fn in (eng.value_backward, eng.policy_forward, eng.policy_backward, eng.step, eng.policy_only, eng.policy_only_forward):
            with pytest.raises(N.NativeError, match="goal-conditioned") as ei:
                fn(hp)
            assert "rc=-1" in str(ei.value) and "porl_iql_" in str(ei.value)
        with pytest.raises(N.NativeError, match="goal-conditioned"):
            eng.policy_prefetch()
        eng.load_batch(z(B, S + G), z(B, S + G), z(B), z(B), z(B, A))          # an ordinary batch: the bc calls refuse it
        torch.cuda.synchronize()
        ws2 = eng.workspace.clone()
        for fn in (eng.bc_step, eng.bc_forward):
            with pytest.raises(N.NativeError, match="porl_iql_load_batch_cat") as ei:
                fn(hp)
            assert fn.__name__ in str(ei.value)
        launched = [p for p in E.prof_read(512) if p["launches"]]
    finally:
        E.prof_enable(False)
    assert launched == [], launched                                            # (load_batch's pack kernel is not a labelled launch)
    assert torch.equal(eng.workspace, ws2) and torch.equal(eng.params_pol, pol)
    assert bool((eng.stats == 7.0).all())
    assert not torch.equal(ws, ws2)                                            # the second load did stage something
    eng.load_batch_cat(z(B, S), z(B, G), z(B, A))
    eng.bc_forward(hp)
    eng.policy_backward(hp)                                                    # completes bc_forward: allowed
    assert np.isfinite(eng.stats[1:3].tolist()).all()


def test_a_rejected_update_moves_no_counter():
    S, A = 20, 3
    rows, r1, _ = _replays(S, A, n=300)
    bc, twin = _make_bc(S, S, A, B=32), _make_bc(S, S, A, B=32)
    for m in (bc, twin):
        m.update_from_replay(r1 if m is bc else _replays(S, A, n=300)[1], 32)
    before = {k: v.clone() for k, v in bc.state_dict().items()}
    big = torch.zeros(33, 2 * S + 2 + A, device=DEV)
    with pytest.raises(RuntimeError):
        bc.update(big[:, :S], big[:, S + 1:2 * S + 1], big[:, 2 * S + 2:])      # max_batch is 32
    with pytest.raises(RuntimeError):
        bc.update_from_replay(r1, 33)
    with pytest.raises(ValueError):
        small = SimpleNamespace(rows=r1.rows[:20], obs_dim=S, act_dim=A, seed=1, draws=0)
        bc.update_from_replay(small, 32)                                        # 32 distinct rows of 20
    with pytest.raises(ValueError):
        bc.update_from_replay(r1, 8, goal="nearest")
    with pytest.raises(ValueError):
        bc.update_from_replay(r1, 8, goal="hindsight", indices=torch.arange(8, device=DEV))
    assert r1.draws == 1 and bc.policy_optimizer.step_count == 1 and bc.policy_lr_schedule.last_epoch == 1
    for k, v in bc.state_dict().items():
        assert torch.equal(v, before[k]), k
    _assert_same(bc, twin)


# ---- 6: POR acts through it ------------------------------------------------------------------------------------------------
def test_por_select_action_and_evaluate_por_act_through_the_policy():
    from porl_amd.agent.por import POR
    from porl_amd.util.util import evaluate_por
    S, A, H, L = 12, 2, 32, 2
    torch.manual_seed(0)
    agent = POR(SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=L, layer_norm=False, action_size=A, max_batch=64),
                1000, 0.9, 10.0, device=DEV)
    bc = _make_bc(S, S, A, H, L, B=64, seed=1)
    rows, r1, _ = _replays(S, A, n=600)
    for _ in range(3):
        bc.update_from_replay(r1, 64)
        agent.update_from_replay(r1, 64)
    keys = list(agent.state_dict().keys())
    assert len(keys) == 31
    with pytest.raises(RuntimeError, match="set_execute_policy"):
        agent.select_action(np.zeros(S, np.float32))
    agent.set_execute_policy(bc)
    assert list(agent.state_dict().keys()) == keys
    # the oracle's two chained means
    Pg = {k: v for k, v in _np_sd(agent).items()}
    Pb = _np_sd(bc)
    obs = make_rows(5, S, A, seed=9)[:, :S]
    goal, _ = O.mlp_forward(Pg, "goal_policy.net", obs, L, False, None)
    want, _ = O.mlp_forward(Pb, "policy.net", np.concatenate([obs, goal], axis=1), L, False, None)
    got = agent.select_action(obs)
    assert isinstance(got, np.ndarray) and got.shape == (5, A) and got.dtype == np.float32
    np.testing.assert_allclose(got, want, atol=1e-5, rtol=0)
    np.testing.assert_allclose(agent.select_action(obs[0]), want[0], atol=1e-5, rtol=0)
    np.testing.assert_allclose(agent.select_action(torch.from_numpy(obs).to(DEV)), want, atol=1e-5, rtol=0)
    # evaluate_por rolls out the same two policies: the actions the environment receives are select_action's
    env = _RolloutEnv(S, A)
    ret = evaluate_por(env, bc.policy, agent.goal_policy, np.zeros(S, np.float32), np.ones(S, np.float32))
    assert np.isfinite(ret) and 1 <= len(env.actions) == len(env.observations) - 1
    for o, act in zip(env.observations, env.actions):
        assert act.shape == (A,)
        np.testing.assert_allclose(act, agent.select_action(o), atol=1e-5, rtol=0)


class _RolloutEnv:
    """tests/helpers/online_env.py's ToyEnv behind the protocol the evaluators speak (reset() -> observation, step(a) ->
    four values, a continuous action): the toy dynamics take the index of the action's largest entry.  Records what the
    loop saw and sent."""

    def __init__(self, S, A):
        from helpers.online_env import ToyEnv
        self.env = ToyEnv(seed=3, state_size=S, action_size=A, max_len=9)
        self.observations, self.actions = [], []

    def reset(self):
        o, _ = self.env.reset()
        self.observations.append(o)
        return o

    def step(self, action):
        self.actions.append(np.array(action, copy=True))
        o, r, terminated, truncated, _ = self.env.step(int(np.argmax(action)))
        self.observations.append(o)
        return o, r, terminated or truncated, {}
