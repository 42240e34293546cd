"""The IQL engine's forward-only entry points (porl_iql_forward_value / porl_iql_forward_policy: TwinV.both,
GaussianPolicy.forward / act / mean_numpy, SORL.select_action, the rollout path forward_policy_host) against the fp64
oracle over the grid of tests/helpers/forward_cases.py.  GPU only.

Engines carry filled parameters (non-zero biases, LayerNorm affine, a target twin of its own); every parameter arena is
prefilled with a finite sentinel so that the 16-byte padding between tensors holds 1e4, and so is the workspace.  A
padding element that is loaded and deselected or multiplied by an exact zero is fine; one that reaches an output moves
it by orders of magnitude.

The bar (forward_cases.reference): error = max |got - ref64| / max(1, max |ref64|) must stay within
max(2e-6, 4 x e32), e32 being the same error of the numpy fp32 oracle on the same parameters and rows.  The defects
these tests exist for (wrong arena, dropped bias, missing tanh, unmasked padding column, stale row) move an output by
1e-3 of scale or more.

Measured on an MI355X at the widest hidden sizes, the only ones where 4 x e32 was expected to exceed 2e-6 (largest
figure over the five outputs and B in {1, 8, 9}; the bar is per output):
  s64_h2048_l2_d6_ln    e32 5.63e-07 (tgt2, bar 2.25e-06)   kernel 1.17e-06 (mean at B = 9, bar 2.00e-06)
  s60_h2048_l2_d2_tanh  e32 6.94e-07 (mean, bar 2.78e-06)   kernel 9.59e-07 (tgt1 at B = 9, bar 2.00e-06)
  s60_h2052_l2_d2       e32 6.96e-07 (vf1, bar 2.78e-06)    kernel 1.69e-06 (vf1 at B = 8 and 9, bar 2.78e-06)
Everywhere else (hidden <= 260) the kernel's error stayed below 1.3e-06 against bars of 2.00e-06 to 4.67e-06.
"""
import contextlib
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import forward_cases as FC
from porl_amd import _native as N
from porl_amd import engine as E
from porl_amd.engine import IqlEngine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = 1.0e4
NAMES = [c.name for c in FC.CASES]
STATE = ("params_vf", "params_tgt", "params_pol", "grads_vf", "grads_pol", "adam_m_vf", "adam_v_vf", "adam_m_pol",
         "adam_v_pol", "stats")


def make_engine(case, max_batch=None, sentinel_state=True):
    """A fresh engine with forward_cases.fill written through the tensor table into sentinel-filled arenas."""
    eng = IqlEngine(case.S, case.D, case.H, case.L, case.layer_norm, case.pol_tanh,
                    max_batch=case.max_batch if max_batch is None else max_batch, device=DEV)
    _, arrays, _, _ = FC.case_data(case.name)
    for flat, group, g in ((eng.params_vf, "vf", 0), (eng.params_tgt, "v_target", 0), (eng.params_pol, "policy", 1)):
        flat.fill_(SENTINEL)
        table, tensors = eng.tensor_table(g), FC.group_tensors(case, arrays, group)
        assert [shape for _, shape in table] == [t.shape for t in tensors]
        for view, t in zip(IqlEngine.views(flat, table), tensors):
            view.copy_(torch.from_numpy(t))
    if sentinel_state:                      # a forward that wrote zeros into zero-initialised state would go unseen
        for name in STATE[3:]:
            getattr(eng, name).fill_(SENTINEL)
    eng._ensure_bound()
    eng.workspace.fill_(SENTINEL)
    return eng


@lru_cache(maxsize=None)
def shared_engine(name):
    return make_engine(FC.BY_NAME[name])


@lru_cache(maxsize=None)
def rows(name):
    return torch.from_numpy(FC.case_data(name)[3]).to(DEV)


@contextlib.contextmanager
def nothing_else_moves(eng):
    before = {k: getattr(eng, k).clone() for k in STATE}
    yield
    for k, v in before.items():
        assert torch.equal(getattr(eng, k), v), f"{k} changed during a forward"


def forwards(eng, x):
    """The five outputs of forward_cases.OUTPUTS as device tensors."""
    v1, v2 = eng.forward_value(x)
    t1, t2 = eng.forward_value(x, target=True)
    return dict(zip(FC.OUTPUTS, (v1, v2, t1, t2, eng.forward_policy(x))))


def check(got, ref, what):
    worst = []
    for k in FC.OUTPUTS:
        err = FC.error(got[k].cpu().numpy(), ref["ref"][k])
        print(f"{what} {k}: error {err:.2e}  e32 {ref['e32'][k]:.2e}  bar {ref['bar'][k]:.2e}")
        if not err <= ref["bar"][k]:
            worst.append((k, err, ref["bar"][k]))
    assert not worst, f"{what}: over the bar: {worst}"


def same_bits(a, b, what):
    for k in FC.OUTPUTS:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs by {(a[k] - b[k]).abs().max().item():.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_grid_matches_the_fp64_oracle(name):
    case, eng, x = FC.BY_NAME[name], shared_engine(name), rows(name)
    with nothing_else_moves(eng):
        for B in case.batches:
            got = forwards(eng, x[:B])
            ref = FC.reference(name, B)
            check(got, ref, f"{name} B={B}")
            # the test cannot pass by reading one arena twice
            for a, b in (("vf1", "tgt1"), ("vf2", "tgt2")):
                assert FC.error(got[a].cpu().numpy(), got[b].cpu().numpy()) > 1e-2, (a, b)
            if B <= IqlEngine.SMALL_BATCH:          # the rollout path: same launches, pinned host memory at both ends
                want = got["mean"].cpu().numpy()
                for src in (x[:B], x[:B].cpu(), x[:B].cpu().numpy()):
                    np.testing.assert_array_equal(eng.forward_policy_host(src), want)


def _profiled(fn):
    E.prof_enable(True)
    try:
        fn()
        prof = E.prof_read(512)
    finally:
        E.prof_enable(False)
    counts = {}
    for p in prof:
        if p["launches"]:
            k = FC.GEMM if p["name"].startswith(FC.GEMM) else p["name"]
            counts[k] = counts.get(k, 0) + p["launches"]
    return counts


@pytest.mark.parametrize("name", NAMES)
def test_the_chosen_kernels_are_the_expected_ones(name):
    """The launches the profiler labels (small_fwd_kernel, l0_fwd_kernel, mean_skinny_kernel, the grouped GEMM) are
    exactly those forward_cases.expected_kernels predicts from the shape, by name and by count."""
    case, eng, x = FC.BY_NAME[name], shared_engine(name), rows(name)
    for B in case.batches:
        for which, fn in (("vf", lambda: eng.forward_value(x[:B])),
                          ("v_target", lambda: eng.forward_value(x[:B], target=True)),
                          ("policy", lambda: eng.forward_policy(x[:B]))):
            assert _profiled(fn) == FC.labelled_counts(case, B, which), (name, B, which)


@pytest.mark.parametrize("name", NAMES)
def test_rows_of_a_nine_row_call_equal_the_eight_row_call(name):
    """B = 8 | 9 is the switch between the GEMV family and the batched kernels."""
    eng, x = shared_engine(name), rows(name)
    ref = FC.reference(name, 8)
    g8, g9 = forwards(eng, x[:8]), forwards(eng, x[:9])
    for k in FC.OUTPUTS:
        err = FC.error(g9[k][:8].cpu().numpy(), g8[k].cpu().numpy().astype(np.float64))
        print(f"{name} {k}: 9-row against 8-row {err:.2e}  bar {ref['bar'][k]:.2e}")
        assert err <= ref["bar"][k], k


@pytest.mark.parametrize("name", NAMES)
def test_strided_input_rows_are_read_in_place(name):
    """A column slice of a packed (B, S + 5) matrix: the small path reads it with its row stride, the batched path hands
    the stride to pack_kernel."""
    case, eng, x = FC.BY_NAME[name], shared_engine(name), rows(name)
    for B in (7, 65 if case.max_batch >= 65 else 9):
        packed = torch.full((B, case.S + 5), SENTINEL, device=DEV)
        packed[:, :case.S] = x[:B]
        view = packed[:, :case.S]
        assert not view.is_contiguous() or B == 1
        same_bits(forwards(eng, view), forwards(eng, view.contiguous()), f"{name} B={B}")
        same_bits(forwards(eng, view), forwards(eng, x[:B]), f"{name} B={B} against the plain rows")


@pytest.mark.parametrize("name", ["s60_h48_l2_d2", "s17_h48_l3_d6_ln"])
def test_scratch_left_by_a_larger_batch_is_not_read(name):
    case, x = FC.BY_NAME[name], rows(name)
    eng = make_engine(case)
    for B in (130, 1, 65, 8, 9):
        same_bits(forwards(eng, x[:B]), forwards(make_engine(case), x[:B]), f"{name} B={B} after larger batches")


def _batch(case, B, seed=5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g).to(DEV)
    term = (torch.rand(B, generator=g) < 0.1).float().to(DEV)
    return r(B, case.S), r(B, case.S), r(B), term, r(B, case.D)


def _state(eng):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).clone() for k in STATE}


def test_small_forwards_between_load_and_step_leave_the_update_alone():
    case = FC.BY_NAME["s60_h48_l2_d2"]
    x = rows(case.name)
    out = []
    for with_forwards in (False, True):
        eng = make_engine(case, sentinel_state=False)
        hp = eng.hyper(inv_batch=1.0 / 64, value_lr=1e-3, policy_lr=1e-3)
        eng.load_batch(*_batch(case, 64))
        if with_forwards:
            check(forwards(eng, x[:8]), FC.reference(case.name, 8), "between load and step")
        eng.step(hp)
        out.append(_state(eng))
    assert torch.isfinite(out[0]["stats"][:3]).all() and not torch.equal(out[0]["params_vf"], shared_engine(case.name).params_vf)
    for k in STATE:
        assert torch.equal(out[0][k], out[1][k]), f"{k}: an 8-row forward between load_batch and step changed the update"


def test_a_batched_forward_invalidates_the_loaded_minibatch_and_says_so():
    case = FC.BY_NAME["s60_h48_l2_d2"]
    eng = make_engine(case, sentinel_state=False)
    hp = eng.hyper(inv_batch=1.0 / 64)
    eng.load_batch(*_batch(case, 64))
    before = _state(eng)
    eng.forward_value(rows(case.name)[:9])          # overwrites the s' staging buffer
    with pytest.raises(N.NativeError, match="no minibatch loaded"):
        eng.step(hp)
    after = _state(eng)
    for k in STATE[:3]:
        assert torch.equal(before[k], after[k]), k


def test_eight_rows_too_wide_for_the_small_path_fall_through_to_the_batched_one():
    """8 rows of 2052 floats exceed the 64 KiB of LDS the small path stages a layer's input in: both entry points take
    their batched path, decided before the first launch (7 rows and 9 rows always worked)."""
    name = "s60_h2052_l2_d2"
    case, eng, x = FC.BY_NAME[name], shared_engine(name), rows(name)
    assert case.max_batch >= 9 and not FC.small_path(case, 8, "policy") and not FC.small_path(case, 8, "vf")
    ref8 = FC.reference(name, 8)
    with nothing_else_moves(eng):
        g8 = forwards(eng, x[:8])
        check(g8, ref8, f"{name} B=8")
        host = eng.forward_policy_host(x[:8].cpu().numpy())
        assert FC.error(host, ref8["ref"]["mean"]) <= ref8["bar"]["mean"]
        np.testing.assert_array_equal(host, g8["mean"].cpu().numpy())
        np.testing.assert_array_equal(eng.forward_policy_host(x[:8]), host)
        g9 = forwards(eng, x[:9])
        for k in FC.OUTPUTS:
            assert FC.error(g9[k][:8].cpu().numpy(), g8[k].cpu().numpy().astype(np.float64)) <= ref8["bar"][k], k
        check(forwards(eng, x[:7]), FC.reference(name, 7), f"{name} B=7")      # still the small path


def test_a_batch_above_max_batch_is_refused_by_both_paths():
    """The small-batch branches used to run before the batch <= max_batch check of the batched path and wrote 8 rows of
    activations into scratch sized for 4."""
    case = FC.BY_NAME["s60_h48_l2_d2"]
    x = rows(case.name)
    eng = make_engine(case, max_batch=4)
    with nothing_else_moves(eng):
        for call in (lambda: eng.forward_value(x[:8]), lambda: eng.forward_value(x[:8], target=True),
                     lambda: eng.forward_policy(x[:8]), lambda: eng.forward_policy_host(x[:8]),
                     lambda: eng.forward_policy(x[:9])):
            with pytest.raises(N.NativeError, match=r"outside \[1,4\]"):
                call()
        got = forwards(eng, x[:4])
    same_bits(got, forwards(make_engine(case, max_batch=4), x[:4]), "4 rows after the refused calls")
    check(got, FC.reference(case.name, 4), "max_batch=4 B=4")


# ---- agent level -----------------------------------------------------------------------------------------------------
def _args(S, H, L, ln, A, B):
    return SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=L, layer_norm=ln, feature_dim=256, action_size=A,
                           max_batch=B)


def _np_sd(agent):
    return {k: v.detach().cpu().numpy() for k, v in agent.state_dict().items()}


def test_por_modules_after_two_updates_match_the_oracle():
    """Two real updates separate the target twin from the online one (Adam on vf, EMA on v_target)."""
    from porl_amd.agent.por import POR
    from porl_amd.util.synth import make_rows, split_rows
    S, H, L = 17, 48, 3
    case = FC.Case("por", S, S, H, L, True, False, 64, ())
    torch.manual_seed(11)
    agent = POR(_args(S, H, L, True, 2, 64), 1000, 0.9, 10.0, device=DEV, value_lr=1e-2)
    data = torch.from_numpy(make_rows(128, S, 2, seed=13)).to(DEV)
    for k in range(2):
        s, r, sp, d, _ = split_rows(data[64 * k:64 * (k + 1)], S, 2)
        agent.por_residual_update(s, sp, r, d)
    P = _np_sd(agent)
    xs = torch.from_numpy(make_rows(40, S, 2, seed=17)[:, :S].copy()).to(DEV)
    for B in (5, 40):
        x = xs[:B]
        ref = FC.reference_for(case, P, x.cpu().numpy())
        v1, v2 = agent.vf.both(x)
        t1, t2 = agent.v_target.both(x)
        got = dict(zip(FC.OUTPUTS, (v1, v2, t1, t2, agent.goal_policy(x).mean)))
        check(got, ref, f"POR B={B}")
        vmin = np.minimum(ref["ref"]["vf1"], ref["ref"]["vf2"])
        assert FC.error(agent.vf(x).cpu().numpy(), vmin) <= max(ref["bar"]["vf1"], ref["bar"]["vf2"])
        for a, b in (("vf1", "tgt1"), ("vf2", "tgt2")):
            assert FC.error(got[a].cpu().numpy(), got[b].cpu().numpy()) > 1e-3, "the target has not left the online twin"


@pytest.mark.parametrize("D", [2, 6])
def test_sorl_select_action_matches_the_oracle(D):
    import oracle.por_oracle as O
    from porl_amd.agent.sorl import SORL
    from porl_amd.util.synth import make_rows
    S, H, L = 60, 64, 2
    torch.manual_seed(3 + D)
    agent = SORL(_args(S, H, L, False, D, 64), 1000, 0.9, 10.0, device=DEV)
    P = _np_sd(agent)
    xs = torch.from_numpy(make_rows(9, S, D, seed=19)[:, :S].copy()).to(DEV)

    def oracle_mean(dtype, x):
        O.set_precision(dtype)
        try:
            return O.sorl_oracle({k: np.asarray(v, dtype) for k, v in P.items()}, S, H, L).select_action(x.astype(dtype))
        finally:
            O.set_precision(np.float32)

    for B in (1, 8, 9):
        x = xs[:B]
        xn = x.cpu().numpy()
        ref64 = oracle_mean(np.float64, xn)
        bar = max(FC.BAR_FLOOR, FC.BAR_FACTOR * FC.error(oracle_mean(np.float32, xn), ref64))
        got = agent.select_action(x)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (B, D)
        err = FC.error(got, ref64)
        print(f"SORL D={D} B={B}: error {err:.2e} bar {bar:.2e}")
        assert err <= bar and np.abs(ref64).max() < 1
        want = agent.policy(x).mean.cpu().numpy()
        for src in (x, x.cpu(), xn):
            np.testing.assert_array_equal(agent.policy.mean_numpy(src), want)
