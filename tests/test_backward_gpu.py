"""The IQL engine's backward phases (porl_iql_value_backward, porl_iql_policy_backward, porl_iql_policy_only_forward:
relu_head_bwd_kernel, value_loss_kernel, ln_relu_bwd_kernel, policy_weight_kernel, policy_nll_kernel, the three kernels
of csrc/skinny.hpp and the slab combines of multi_reduce_kernel) per element against the fp64 oracle over the grid of
tests/helpers/backward_cases.py.  GPU only.

Batches hold DECIDED rows only (no ReLU of a net that receives gradients within 1e-4 of its kink in fp64), so no element
is excused: every gradient tensor of both groups and stats[0:3] must be within max(2e-6, 4 x e32) of the fp64 result,
error = max |got - ref64| / max |ref64| over the tensor and e32 the same error of the numpy fp32 run.  d/dlog_std of an
entry outside [-5, 2] must be exactly zero, and so must every tensor whose reference is zero.  Engines carry
forward_cases.fill's parameters in sentinel-filled arenas; gradient arenas, Adam moments, statistics and the whole
workspace hold 1e4 before load_batch, so a padding column that a skinny kernel reads without its producer having zeroed
it, or a ragged tile that writes past its tensor, shows.

No kernel or host defect turned up: nothing here motivated a change under porl_amd/.  What failed at first were the
inputs: with a policy mean of O(1) in a column with sigma = e^-5, single policy tensors landed at 5 x the numpy run's
error, and the numpy run at 5 x the kernel's on others; backward_cases.params says why and what it does about it.

Measured on an MI355X, the output closest to its bar per configuration (over its batches, both weight modes, the joint
and the policy-only run and every tune variant; the bar is per output):
  s60_h48_l2_d2           goal_policy.net.0.bias    e32 2.24e-07  kernel 9.51e-07  bar 2.00e-06  (B = 65, mode 1)
  s1_h48_l1_d1_tanh       goal_policy.net.2.bias    e32 9.18e-08  kernel 5.00e-07  bar 2.00e-06  (B = 65, mode 0)
  s3_h30_l2_d6_tanh       goal_policy.net.2.weight  e32 2.50e-07  kernel 6.88e-07  bar 2.00e-06  (B = 1, mode 0)
  s17_h48_l3_d6_ln        goal_policy.log_std       e32 6.15e-07  kernel 2.14e-06  bar 2.46e-06  (B = 9, mode 0)
  s64_h132_l2_d64_tanh    goal_policy.net.0.weight  e32 3.56e-07  kernel 1.11e-06  bar 2.00e-06  (B = 1, mode 0)
  s68_h132_l1_d65         goal_policy.log_std       e32 4.15e-07  kernel 1.18e-06  bar 2.00e-06  (B = 9, mode 0)
  s364_h48_l2_d70_tanh    goal_policy.net.2.weight  e32 3.79e-07  kernel 1.37e-06  bar 2.00e-06  (B = 9, mode 1)
  s60_h260_l2_d2_ln_tanh  goal_policy.log_std       e32 5.63e-07  kernel 1.13e-06  bar 2.25e-06  (B = 9, mode 1)
  s64_h2048_l2_d6_ln      vf.v1.1.bias              e32 5.32e-07  kernel 2.05e-06  bar 2.13e-06  (B = 1, mode 0)
  s60_h2048_l2_d2_tanh    vf.v2.0.weight            e32 4.03e-07  kernel 1.83e-06  bar 2.00e-06  (B = 1, mode 0)
  s60_h2052_l2_d2         stats1                    e32 1.39e-07  kernel 1.34e-06  bar 2.00e-06  (B = 1, mode 0)
  s17_h30_l1_d65_ln_tanh  goal_policy.net.2.bias    e32 4.21e-07  kernel 5.20e-07  bar 2.00e-06  (B = 65, mode 1)
  s60_h64_l3_d1           goal_policy.log_std       e32 3.98e-07  kernel 1.15e-06  bar 2.00e-06  (B = 9, mode 1)
  s3_h132_l3_d70_tanh     stats0                    e32 8.81e-07  kernel 2.41e-06  bar 3.52e-06  (B = 1, mode 0)
  s68_h260_l1_d64_ln      goal_policy.net.2.bias    e32 4.55e-07  kernel 7.55e-07  bar 2.00e-06  (B = 65, mode 1)
  s1_h30_l3_d2_ln_tanh    goal_policy.net.0.weight  e32 7.38e-07  kernel 1.50e-06  bar 2.95e-06  (B = 1, mode 0)
  s60_h580_l1_d6          goal_policy.net.2.bias    e32 4.66e-07  kernel 1.07e-06  bar 2.00e-06  (B = 1030, mode 0)
  s60_h1028_l1_d2         vf.v1.2.bias              e32 1.58e-06  kernel 1.96e-06  bar 6.32e-06  (B = 9, mode 0)
The value group's tensors and stats[0] stay below 9e-07 wherever hidden <= 580, except s3_h132_l3_d70_tanh at B = 1
(2.41e-06, its e32 8.81e-07); no factor was raised.  The 265 cases take 8 s.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from helpers import backward_cases as BC
from porl_amd import engine as E
from porl_amd.engine import IqlEngine

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENTINEL = 1.0e4
RUN_IDS = [BC.run_id(r) for r in BC.RUNS]
FROZEN = ("params_vf", "params_tgt", "params_pol", "adam_m_vf", "adam_v_vf", "adam_m_pol", "adam_v_pol")
SCRATCH = ("grads_vf", "grads_pol", "stats")


@lru_cache(maxsize=None)
def shared_engine(name, max_batch, weight_mode):
    """An engine with backward_cases.params written through the tensor table into sentinel-filled arenas."""
    case, arrays, _ = BC.params(name)
    eng = IqlEngine(case.S, case.D, case.H, case.L, case.layer_norm, case.pol_tanh, weight_mode=weight_mode,
                    max_batch=max_batch, device=DEV)
    for flat, group, g in ((eng.params_vf, "vf", 0), (eng.params_tgt, "v_target", 0), (eng.params_pol, "policy", 1)):
        flat.fill_(SENTINEL)
        table, tensors = eng.tensor_table(g), BC.FC.group_tensors(case, arrays, group)
        assert [shape for _, shape in table] == [t.shape for t in tensors]
        for view, t in zip(IqlEngine.views(flat, table), tensors):
            view.copy_(torch.from_numpy(np.array(t)))      # a copy: the cached arrays are read-only
    for k in FROZEN[3:]:
        getattr(eng, k).fill_(SENTINEL)
    eng._ensure_bound()
    return eng


@lru_cache(maxsize=None)
def rows(name, B):
    return tuple(torch.from_numpy(np.array(a)).to(DEV) for a in BC.batch(name, B))


@lru_cache(maxsize=None)
def in_no_tensor(name, group):
    """Boolean mask over a gradient arena: the elements that belong to no tensor (padding between tensors, the tail)."""
    eng = shared_engine(name, *[(r.max_batch, 0) for r in BC.RUNS if r.name == name][0])
    flat = eng.grads_vf if group == 0 else eng.grads_pol
    mask = torch.ones(flat.numel(), dtype=torch.bool, device=DEV)
    for off, shape in eng.tensor_table(group):
        mask[off:off + int(np.prod(shape))] = False
    return mask


def hyper(eng, B, mode):
    return eng.hyper(tau=BC.TAU, discount=BC.DISCOUNT, alpha=BC.ALPHA[mode], inv_batch=1.0 / B)


def read_group(eng, case, group):
    flat = eng.grads_vf if group == 0 else eng.grads_pol
    names, views = BC.tensor_names(case, group), IqlEngine.views(flat, eng.tensor_table(group))
    assert len(names) == len(views)
    return {n: v.cpu().numpy().copy() for n, v in zip(names, views)}


class Phases:
    """One run of the phases on a shared engine: sentinels before load_batch, `tune` for its duration, and on the way out
    the checks that hold for every run — nothing but gradients and statistics moved, no arena element outside a tensor
    was written."""

    def __init__(self, run, mode, tune=(), engine_mode=0):
        self.run, self.mode, self.case = run, mode, BC.BY_NAME[run.name]
        self.eng = shared_engine(run.name, run.max_batch, mode)
        self.tune, self.engine_mode = tuple(run.tune) + tuple(tune), engine_mode
        self.hp = hyper(self.eng, run.B, mode)

    def __enter__(self):
        eng = self.eng
        for k in SCRATCH:
            getattr(eng, k).fill_(SENTINEL)
        eng.workspace.fill_(SENTINEL)
        self.before = {k: getattr(eng, k).clone() for k in FROZEN}
        for k, v in self.tune:
            eng.tune_set(k, v)
        eng.set_mode(self.engine_mode)
        eng.load_batch(*rows(self.run.name, self.run.B))
        return self

    def __exit__(self, exc_type, exc, tb):
        eng = self.eng
        eng.set_mode(0)
        for k, _ in self.tune:
            eng.tune_set(k, {"skinny": BC.SKINNY_DEFAULT, "dw0_slabs": BC.DW0_SLABS_DEFAULT}[k])
        if exc_type is not None:
            return False
        torch.cuda.synchronize()
        for k, v in self.before.items():
            assert torch.equal(getattr(eng, k), v), f"{k} changed during a backward phase"
        for group, flat in ((0, eng.grads_vf), (1, eng.grads_pol)):
            pad = flat[in_no_tensor(self.run.name, group)]
            assert bool((pad == SENTINEL).all()), f"group {group}: {int((pad != SENTINEL).sum())} padding elements written"
        assert bool((eng.stats[3:] == SENTINEL).all()), "stats[3:] written"
        return False

    def value(self):
        self.eng.value_backward(self.hp)
        return read_group(self.eng, self.case, 0), self.eng.stats[:1].cpu().numpy().copy()

    def policy(self):
        self.eng.policy_backward(self.hp)
        return read_group(self.eng, self.case, 1), self.eng.stats[1:3].cpu().numpy().copy()

    def joint(self):
        """load -> value_backward -> policy_backward, no apply in between: the policy phase reads the un-updated twins and
        the value phase's target_v, as backward_cases._phases does."""
        g0, s0 = self.value()
        g1, s12 = self.policy()
        return dict(grads={**g0, **g1}, stats=np.concatenate([s0, s12]))

    def policy_only(self):
        """policy_only_forward, then policy_backward, which runs the gradient half only; the value group is not written."""
        self.eng.policy_only_forward(self.hp)
        g1, s12 = self.policy()
        assert bool((self.eng.grads_vf == SENTINEL).all()) and float(self.eng.stats[0]) == SENTINEL
        return dict(grads=g1, stats=np.concatenate([[np.float32("nan")], s12]))


def check(got, run, mode, what, groups=(0, 1)):
    ref = BC.reference(run.name, run.B, mode)
    case = BC.BY_NAME[run.name]
    keys = [n for g in groups for n in BC.tensor_names(case, g)] + [f"stats{i}" for i in range(3) if i > 0 or 0 in groups]
    over = []
    for k in keys:
        if k.startswith("stats"):
            i = int(k[5:])
            err = BC.tensor_error(got["stats"][i], ref["ref"]["stats"][i])
        else:
            assert got["grads"][k].dtype == np.float32
            err = BC.tensor_error(got["grads"][k], ref["ref"]["grads"][k])
        print(f"{what} w{mode} {k}: error {err:.2e}  e32 {ref['e32'][k]:.2e}  bar {ref['bar'][k]:.2e}")
        if not err <= ref["bar"][k]:
            over.append((k, err, ref["bar"][k]))
    assert not over, f"{what} w{mode}: over the bar: {over}"
    if 1 in groups:
        out = BC.clamped_out(run.name)
        assert not got["grads"]["goal_policy.log_std"][out].any(), "d/dlog_std outside [-5, 2] is not exactly zero"


def same_bits(a, b, what):
    for k in a["grads"]:
        assert np.array_equal(a["grads"][k], b["grads"][k]), f"{what}: {k} differs"
    assert np.array_equal(a["stats"], b["stats"], equal_nan=True), f"{what}: stats differ"


def profiled(fn):
    """-> (fn's result, {skinny kernel: launches})"""
    E.prof_enable(True)
    try:
        out = fn()
        prof = E.prof_read(512)
    finally:
        E.prof_enable(False)
    counts = {}
    for p in prof:
        for k in BC.SKINNY_KERNELS:
            if p["launches"] and p["name"].endswith(k):
                counts[k] = counts.get(k, 0) + p["launches"]
    return out, counts


def merged(*dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = out.get(k, 0) + v
    return out


# ---- the grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BC.WEIGHT_MODES)
@pytest.mark.parametrize("rid", RUN_IDS)
def test_joint_gradients_match_the_fp64_oracle(rid, mode):
    run = BC.RUNS[RUN_IDS.index(rid)]
    with Phases(run, mode) as ph:
        got, counts = profiled(ph.joint)
        check(got, run, mode, rid)
        skinny = dict(run.tune).get("skinny", BC.SKINNY_DEFAULT)
        assert counts == merged(BC.skinny_kernels(ph.case, "value", skinny), BC.skinny_kernels(ph.case, "policy", skinny)), rid


@pytest.mark.parametrize("mode", BC.WEIGHT_MODES)
@pytest.mark.parametrize("rid", RUN_IDS)
def test_policy_only_gradients_match_the_fp64_oracle(rid, mode):
    """Weights from the TD target (policy_weight_kernel) instead of the value phase's target_v: the same numbers in exact
    arithmetic, from five forward-only nets."""
    run = BC.RUNS[RUN_IDS.index(rid)]
    with Phases(run, mode) as ph:
        got, counts = profiled(ph.policy_only)
        check(got, run, mode, rid + " policy-only", groups=(1,))
        assert counts == merged(BC.skinny_kernels(ph.case, "forward"), BC.skinny_kernels(ph.case, "gradient")), rid


# ---- tune variants -----------------------------------------------------------------------------------------------------
SKINNY_RUNS = [("s60_h48_l2_d2", 130), ("s60_h48_l2_d2", BC.BIG), ("s64_h132_l2_d64_tanh", 65), ("s17_h48_l3_d6_ln", 65),
               ("s60_h2052_l2_d2", 9), ("s60_h1028_l1_d2", 9), ("s60_h580_l1_d6", BC.BIG)]


def _run(name, B):
    return next(r for r in BC.RUNS if r.name == name and r.B == B and not r.tune)


@pytest.mark.parametrize("skinny", [0, 1, 2, 4, 7])
@pytest.mark.parametrize("name,B", SKINNY_RUNS)
def test_each_skinny_kernel_and_its_gemm_path_match_the_oracle(name, B, skinny):
    """`skinny` is a bit mask (1 dW0, 2 policy mean, 4 policy output layer; porl_tune_set reads the value 1 as "all"):
    every product is compared with the oracle on its skinny kernel and on the grouped GEMM, and the profiler shows that
    exactly the expected ones of the three kernels were launched — a silent fall-back does not pass."""
    run = _run(name, B)
    for mode in BC.WEIGHT_MODES:
        with Phases(run, mode, tune=(("skinny", skinny),)) as ph:
            got, counts = profiled(ph.joint)
            check(got, run, mode, f"{name} B={B} skinny={skinny}")
            want = merged(BC.skinny_kernels(ph.case, "value", skinny), BC.skinny_kernels(ph.case, "policy", skinny))
            assert counts == want, (counts, want)
            if skinny in (1, 7):
                assert counts.get(BC.MEAN) == 1 and counts.get(BC.OUTBWD) == 1 and counts.get(BC.WGRAD, 0) >= 1


@pytest.mark.parametrize("slabs", [1, 2, 16])
@pytest.mark.parametrize("name,B", [("s60_h48_l2_d2", 130), ("s60_h48_l2_d2", BC.BIG), ("s17_h48_l3_d6_ln", 130)])
def test_dw0_slab_counts_match_the_oracle(name, B, slabs):
    run = _run(name, B)
    for mode in BC.WEIGHT_MODES:
        with Phases(run, mode, tune=(("dw0_slabs", slabs),)) as ph:
            check(ph.joint(), run, mode, f"{name} B={B} dw0_slabs={slabs}")


@pytest.mark.parametrize("name,B", [("s60_h48_l2_d2", 130), ("s17_h48_l3_d6_ln", 65), ("s60_h2052_l2_d2", 9)])
def test_short_block_mode_matches_the_oracle(name, B):
    """PORL_IQL_MODE_SHORT_BLOCKS, the mode the default pipelined update runs in (other tiles, the value phase's LDS pad,
    the skinny kernels by width: off above hidden 768), through the same phase calls."""
    run = _run(name, B)
    for mode in BC.WEIGHT_MODES:
        with Phases(run, mode, engine_mode=IqlEngine.MODE_SHORT_BLOCKS) as ph:
            got, counts = profiled(ph.joint)
            check(got, run, mode, f"{name} B={B} short blocks")
            assert counts == merged(BC.skinny_kernels(ph.case, "value", short_blocks=True),
                                    BC.skinny_kernels(ph.case, "policy", short_blocks=True))
        with Phases(run, mode, engine_mode=IqlEngine.MODE_SHORT_BLOCKS) as ph:
            check(ph.policy_only(), run, mode, f"{name} B={B} short blocks policy-only", groups=(1,))


# ---- prefetch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("s60_h48_l2_d2", 130), ("s17_h48_l3_d6_ln", 65), ("s68_h132_l1_d65", 65),
                                    ("s3_h30_l2_d6_tanh", 9), ("s60_h2052_l2_d2", 9)])
def test_policy_prefetch_before_the_value_phase_changes_no_bit(name, B):
    run = _run(name, B)
    for mode in BC.WEIGHT_MODES:
        with Phases(run, mode) as ph:
            plain = ph.joint()
        with Phases(run, mode) as ph:
            ph.eng.policy_prefetch()
            g0, s0 = ph.value()
            g1, s12 = ph.policy()
            pre = dict(grads={**g0, **g1}, stats=np.concatenate([s0, s12]))
        same_bits(plain, pre, f"{name} B={B} w{mode}: policy_prefetch before value_backward")
        with Phases(run, mode) as ph:
            only = ph.policy_only()
        with Phases(run, mode) as ph:
            ph.eng.policy_prefetch()
            only_pre = ph.policy_only()
        same_bits(only, only_pre, f"{name} B={B} w{mode}: policy_prefetch before policy_only_forward")


def test_gradients_do_not_depend_on_what_the_workspace_held():
    """The same run after a larger batch left its rows behind (no sentinel refill in between)."""
    run_small, run_big = _run("s60_h48_l2_d2", 65), _run("s60_h48_l2_d2", 130)
    assert run_small.max_batch == run_big.max_batch
    for mode in BC.WEIGHT_MODES:
        with Phases(run_small, mode) as ph:
            fresh = ph.joint()
        with Phases(run_big, mode) as ph:
            ph.joint()
            ph.eng.load_batch(*rows(run_small.name, run_small.B))
            ph.hp = hyper(ph.eng, run_small.B, mode)
            after = ph.joint()
        same_bits(fresh, after, f"w{mode}: 65 rows after 130")
