"""The Adam launch of the IQL engine with its folded combines (csrc/porl_api.hip: adam_launch; csrc/kernels.hpp:
adam_ema_kernel), driven through porl_amd.engine.IqlEngine on the cases of tests/helpers/adam_cases.FOLD_CASES.

Four engines of one configuration get the same seeded state (parameters, a target that differs from them, moments of a
run in progress, zero gradients), the same batch and the same hyper-parameters, and run one update each:
    step/fold            porl_iql_step, the default: both combines folded into the Adam launches
    step/nofold          tune "iql_fold" = 0: the combines are launches of their own
    phases/foldcombine   PORL_IQL_MODE_FOLD_COMBINE, then value_backward / value_apply / policy_backward / policy_apply
    phases/plain         mode 0, the same four calls
(a) all four leave params_vf, params_tgt, params_pol, grads_vf, grads_pol, the four moment buffers and stats[0:3]
    identical bit for bit — the kernel's claim that folding changes nothing;
(b) on step/fold, parameters and moments against adam64 of (state before, the engine's own completed gradient buffer) and
    params_tgt against ema64 of the new parameters, per element over the whole of both groups, at helpers/adam_cases.BARS;
(c) every float of the nine flat buffers outside the tensors of tensor_table is exactly zero afterwards (the ragged tails
    the skip ranges cover, the slice-quantum tail);
(d) porl_iql_adam_plan reports the plan the case was built for (regions, folded jobs at width 32 / 4, unfolded jobs, skip
    ranges, reduce blocks), and all zeros for the two forms that fold nothing.

What (a) found: ema1 was written `t * omeb + ema_beta * p`, and the compiler contracted it per call site — in the float4
sweep ema_beta * p fused onto the rounded t * omeb, in ema_kernel t * omeb fused onto the rounded ema_beta * p, in the
reduce+Adam branch two rounded products and an add.  So params_tgt could differ in the last bit between the folding and
the non-folding forms on every element a reduce block steps: the twins' output biases (v.b[L]) in every ReLU case, the
head weights (v.w[L]) from 17 head slabs on, everything at H % 4 != 0.  Observed with that form: 7 to 16 floats of the
head weights at 7.5e-9 in slabs17, width4, tiles18, h50 and act4 (the lone bias elements happened to agree).  ema1 and
adam1 now state one explicit form, the sweep's, with __fmaf_rn, and (a) holds.

Asserted plans (regions, folded jobs at width 32, at width 4, unfolded jobs, skip ranges, reduce blocks), re-derived from
HEAD_ROWS, NLL_ROWS_PER_BLOCK, skn_split and pick_splitk as they stand (helpers/adam_cases.FOLD_CASES says what each
case exercises and why three batches differ from a first guess: a grouped-GEMM dW0 leaves a combine only from B = 128):
    d17      S=17  H=48   L=2 B=32    value (6, 2, 0, 1, 2, 3)    policy (3, 2, 0, 2, 2, 4)
    slabs16  S=60  H=64   L=2 B=128   value (6, 2, 0, 1, 2, 3)    policy (4, 1, 0, 2, 1, 4)
    slabs17  S=60  H=64   L=2 B=136   value (4, 4, 0, 1, 4, 7)    policy (4, 1, 0, 2, 1, 4)
    width4   S=60  H=64   L=1 B=520   value (4, 0, 4, 1, 4, 35)   policy (4, 0, 1, 2, 1, 17)
    ln       S=20  H=100  L=2 B=150   value (4, 0, 0, 0, 0, 0)    policy (4, 1, 0, 2, 1, 3)
    tiles18  S=8   H=132  L=3 B=1100  value (4, 0, 4, 1, 4, 69)   policy (4, 0, 1, 2, 1, 4)
    s70      S=70  H=64   L=2 B=128   value (6, 2, 0, 1, 2, 3)    policy (3, 2, 0, 2, 2, 8)
    h50      S=17  H=50   L=2 B=128   value (0, 8, 0, 1, 8, 65)   policy (0, 5, 0, 2, 5, 60)
    act4     S=60  H=64   L=2 B=136   value (4, 4, 0, 1, 4, 7)    policy (4, 1, 0, 2, 1, 3)
H = 50 is not rejected anywhere: porl_iql_create takes it, the odd-width paths of every kernel run, all four checks pass.

Largest observed error over its bar (MI355X), step/fold, over the nine cases; bars not tuned against the kernels:
    value group   params 0.050 (tiles18)   m 0.070 (slabs16)   v 0.013   target 0.082 (slabs16)
    policy group  params 0.049 (tiles18)   m 0.057 (tiles18)   v 0.016 (slabs16)

Hand mutations of csrc/kernels.hpp / csrc/porl_api.hip these tests were tried against, one at a time on a scratch copy
(none changes an address or a bound); "all ReLU cases" = all but `ln`, whose value group has no reduce+Adam block:
    the Polyak line of the reduce+Adam branch dropped      (a) and (b) fail on all ReLU cases (params_tgt)
    the same line reading p from before the step           (a) and (b) fail on all ReLU cases
    ema1 as it was, `t * omeb + ema_beta * p`              (a) fails on slabs17, width4, tiles18, h50, act4: params_tgt of
                                                           both twins' head weights, 7 to 16 floats, by 7.5e-9; the
                                                           bit comparison of tests/test_adam_sweep_gpu.py fails too
    skip_hi without the round-up to 4                      nothing fails, and nothing can: skip_lo is a multiple of 4 and
                                                           the sweep tests float4 starts e = 4 i, for which e < off + n
                                                           and e < ru4(off + n) are the same statement (as are the two
                                                           forms of the block-uniform overlap test).  The round-up
                                                           documents the range; it decides nothing.  (c) pins what it
                                                           is about: the ragged tail stays zero.
    a region's slabs summed sequentially                   (a) fails on slabs16, width4, tiles18, s70 (grads, then all that
                                                           follows): the cases with 9 or 16 slabs in a region.  Up to 8
                                                           slabs the interleaved order IS the sequential one
    `g4[i] = gg` omitted                                   (a) and (b) fail on every case with a region (all but h50)
    bc2_sqrt without the square root                       (b) fails on all nine cases (params, target); 16 sweep rows
    beta2 and omb2 swapped in adam1                        (b) fails on all nine cases (params, v, target); 30 sweep rows
"""
import functools

import numpy as np
import pytest
import torch

from helpers import adam_cases as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FORMS = ("step/fold", "step/nofold", "phases/foldcombine", "phases/plain")
FOLDING = ("step/fold", "phases/foldcombine")
BUFFERS = ("params_vf", "params_tgt", "params_pol", "grads_vf", "grads_pol", "adam_m_vf", "adam_v_vf", "adam_m_pol",
           "adam_v_pol")
GROUP_OF = {"params_vf": 0, "params_tgt": 0, "grads_vf": 0, "adam_m_vf": 0, "adam_v_vf": 0,
            "params_pol": 1, "grads_pol": 1, "adam_m_pol": 1, "adam_v_pol": 1}
NAMES = list(A.FOLD_CASES)


def _write(eng, flat, table, src):
    for view, (off, shape) in zip(eng.views(flat, table), table):
        n = int(np.prod(shape))
        view.copy_(torch.from_numpy(src[off:off + n].reshape(shape)))


def _one(name, form, state, tables, batch):
    from porl_amd.engine import IqlEngine
    S, H, L, B, ln, D = A.FOLD_CASES[name][:6]
    action = name == "act4"
    eng = IqlEngine(S, D, H, L, layer_norm=ln, pol_tanh=action, weight_mode=int(action), max_batch=B, device=DEV)
    if form == "step/nofold":
        eng.tune_set("iql_fold", 0)                     # before binding
    for g, (p, m, v, t) in ((0, ("params_vf", "adam_m_vf", "adam_v_vf", "params_tgt")),
                            (1, ("params_pol", "adam_m_pol", "adam_v_pol", None))):
        _write(eng, getattr(eng, p), tables[g], state[g]["p"])
        _write(eng, getattr(eng, m), tables[g], state[g]["m"])
        _write(eng, getattr(eng, v), tables[g], state[g]["v"])
        if t:
            _write(eng, getattr(eng, t), tables[g], state[g]["t"])
    assert float(eng.grads_vf.abs().sum()) == 0.0 and float(eng.grads_pol.abs().sum()) == 0.0
    before = {k: getattr(eng, k).cpu().numpy().copy() for k in BUFFERS}
    dev = {k: torch.from_numpy(x).to(DEV) for k, x in batch.items()}
    eng.load_batch(dev["obs"], dev["next_obs"], dev["rew"], dev["term"], dev["pol_target"])
    hp = eng.hyper(value_lr=A.LR, policy_lr=A.LR, ema_beta=A.EMA_BETA, value_step=A.VALUE_STEP, policy_step=A.POLICY_STEP,
                   inv_batch=1.0 / B)
    if form.startswith("step/"):
        eng.step(hp)
    else:
        eng.set_mode(eng.MODE_FOLD_COMBINE if form == "phases/foldcombine" else 0)
        eng.value_backward(hp)
        eng.value_apply(hp)
        eng.policy_backward(hp)
        eng.policy_apply(hp)
    torch.cuda.synchronize()
    after = {k: getattr(eng, k).cpu().numpy().copy() for k in BUFFERS}
    after["stats"] = eng.stats[:3].cpu().numpy().copy()
    plans = tuple(tuple(eng.adam_plan(g)[k] for k in A.PLAN) for g in (0, 1))
    assert tuple(eng.adam_plan(0)) == A.PLAN == eng.ADAM_PLAN
    return before, after, plans


@functools.lru_cache(maxsize=None)
def _run(name):
    """One update in each of the four forms -> (tables, state before, {form: buffers after}, {form: plans}); computed once
    per case and shared by the tests below."""
    from porl_amd.engine import IqlEngine
    S, H, L, B, ln, D = A.FOLD_CASES[name][:6]
    probe = IqlEngine(S, D, H, L, layer_norm=ln, max_batch=B, device=DEV)
    tables = {g: probe.tensor_table(g) for g in (0, 1)}
    sizes = {0: probe.params_vf.numel(), 1: probe.params_pol.numel()}
    state = A.fold_state(name, tables, sizes)
    batch = A.fold_batch(name, S, D, B)
    if name == "act4":
        batch["pol_target"] = np.tanh(batch["pol_target"])          # actions lie in (-1, 1)
    before, after, plans = None, {}, {}
    for form in FORMS:
        b, after[form], plans[form] = _one(name, form, state, tables, batch)
        if before is not None:
            for k in BUFFERS:
                assert (b[k].view(np.int32) == before[k].view(np.int32)).all(), f"{form}: {k} started differently"
        before = b
    return tables, before, after, plans


def _tensor_of(tables, buf, i):
    """Name the tensor element i of a flat buffer lies in."""
    for k, (off, shape) in enumerate(tables[GROUP_OF[buf]]):
        if off <= i < off + int(np.prod(shape)):
            return f"tensor {k} {shape} element {i - off}"
    return f"padding at {i}"


@pytest.mark.parametrize("name", NAMES)
def test_forms_are_bit_identical(name):
    tables, before, after, _ = _run(name)
    ref = after[FORMS[0]]
    assert all(np.isfinite(ref[k]).all() for k in ref)
    bad = []
    for form in FORMS[1:]:
        for k in BUFFERS + ("stats",):
            ne = np.flatnonzero(ref[k].view(np.int32) != after[form][k].view(np.int32))
            if ne.size:
                where = sorted({_tensor_of(tables, k, int(i)).split(" element")[0] for i in ne}) if k != "stats" else list(ne)
                bad.append(f"{form} vs {FORMS[0]}: {k} differs in {ne.size} floats ({where}; largest "
                           f"{np.abs(ref[k][ne].astype(np.float64) - after[form][k][ne]).max():.3g})")
    assert not bad, "\n".join(bad)
    # and the update did something everywhere: no tensor element of the value group kept its parameter AND its moments
    for g, (p, m) in ((0, ("params_vf", "adam_m_vf")), (1, ("params_pol", "adam_m_pol"))):
        for off, shape in tables[g]:
            sl = slice(off, off + int(np.prod(shape)))
            assert (ref[m][sl] != before[m][sl]).all(), (g, off, shape)       # m' = 0.9 m + 0.1 g differs from m at any g


@pytest.mark.parametrize("name", NAMES)
def test_per_element_against_the_oracle(name):
    from helpers.qstep_cases import adam64
    tables, before, after, _ = _run(name)
    got = after["step/fold"]
    worst = {}
    for g, (p, m, v, t, gr, step) in ((0, ("params_vf", "adam_m_vf", "adam_v_vf", "params_tgt", "grads_vf", A.VALUE_STEP)),
                                      (1, ("params_pol", "adam_m_pol", "adam_v_pol", None, "grads_pol", A.POLICY_STEP))):
        p64, m64, v64 = adam64(before[p], got[gr], before[m], before[v], lr=A.LR, step=step, betas=A.BETAS, eps=A.EPS)
        e = {"p": A.excess(got[p], p64, "p"), "m": A.excess(got[m], m64, "m"), "v": A.excess(got[v], v64, "v")}
        if t:
            # against the fp64 parameters, not the kernel's: a target computed from wrong parameters is wrong too
            e["t"] = A.excess(got[t], A.ema64(before[t], p64, A.EMA_BETA), "t")
        worst[g] = e
    print(name, worst)
    for g, e in worst.items():
        assert max(e.values()) <= 1.0, (g, e)
    # the policy group has no target, and the value phase's target is the only thing that moved params_tgt
    assert (got["params_tgt"] != before["params_tgt"]).any()


@pytest.mark.parametrize("name", NAMES)
def test_padding_stays_zero(name):
    tables, _, after, _ = _run(name)
    for form in FORMS:
        for k in BUFFERS:
            pad = np.ones(after[form][k].size, dtype=bool)
            for off, shape in tables[GROUP_OF[k]]:
                pad[off:off + int(np.prod(shape))] = False
            assert pad.any()
            nz = np.flatnonzero(pad & (after[form][k] != 0))
            assert nz.size == 0, f"{form}: {k} has {nz.size} non-zero padding floats, first at {nz[:4]}"


@pytest.mark.parametrize("name", NAMES)
def test_the_intended_branch_ran(name):
    _, _, _, plans = _run(name)
    want = A.FOLD_CASES[name][6:8]
    print(name, {f: plans[f] for f in FORMS})
    for form in FORMS:
        assert plans[form] == (want if form in FOLDING else ((0,) * 6, (0,) * 6)), (form, plans[form], want)
