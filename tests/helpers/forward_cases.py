"""Cases of the IQL engine's forward-only entry points (porl_iql_forward_value / porl_iql_forward_policy):
tests/test_forward_cases.py checks them on the CPU, tests/test_forward_gpu.py runs them on the device.

`CASES` are engine configurations with the batch sizes to run, the smallest shapes that reach each branch of the host
code; `expected_kernels` restates that host code's choice of launches in Python; `fill` draws parameters that make
every term of the arithmetic visible (non-zero biases, LayerNorm affine away from (1, 0), a target twin drawn
independently of the online one); `reference` is the fp64 oracle's answer together with the error of the numpy fp32
oracle on the same parameters and rows, from which the tests' bar is derived.  numpy only, no device use.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import por_oracle as O

Case = namedtuple("Case", "name S D H L layer_norm pol_tanh max_batch batches")

# name: s<obs_dim>_h<hidden>_l<n_hidden>_d<policy out>[_ln][_tanh]
CASES = [
    # the plain shape: every K <= 64 layer with a stored output on l0_fwd_kernel, skinny mean, one slab
    Case("s60_h48_l2_d2", 60, 2, 48, 2, False, False, 160, (1, 8, 9, 64, 130)),
    # obs_dim below one 16-byte load; the input layer is also the last one (head fused into a K = 1 product)
    Case("s1_h48_l1_d1_tanh", 1, 1, 48, 1, False, True, 72, (1, 7, 9, 65)),
    # hidden width not a multiple of 4: no l0_fwd_kernel, no mean_skinny_kernel, scalar small_fwd path in every layer
    Case("s3_h30_l2_d6_tanh", 3, 6, 30, 2, False, True, 72, (2, 8, 9, 63)),
    # LayerNorm value nets take the batched path at every batch size; three hidden layers
    Case("s17_h48_l3_d6_ln", 17, 6, 48, 3, True, False, 136, (1, 7, 9, 64, 130)),
    # obs_dim at the l0_fwd_kernel limit, hidden = one 128-column tile + 4, policy width at the skinny limit
    Case("s64_h132_l2_d64_tanh", 64, 64, 132, 2, False, True, 72, (1, 8, 9, 65)),
    # obs_dim just above that limit, policy width just above the skinny limit (split-K GEMM mean, Dp != D), L = 1
    Case("s68_h132_l1_d65", 68, 65, 132, 1, False, False, 72, (2, 8, 9, 63)),
    # obs_dim > 256: a lane of small_fwd_kernel takes a second 16-byte step
    Case("s364_h48_l2_d70_tanh", 364, 70, 48, 2, False, True, 136, (1, 8, 9, 130)),
    # LayerNorm over a second 256-column stride that holds 4 valid columns
    Case("s60_h260_l2_d2_ln_tanh", 60, 2, 260, 2, True, True, 72, (1, 8, 9, 65)),
    # the LayerNorm width limit; 32 K-tiles of the mean in 16 slabs
    Case("s64_h2048_l2_d6_ln", 64, 6, 2048, 2, True, False, 16, (1, 8, 9)),
    # the widest hidden layer whose 8 rows still fit the small path's 64 KiB of LDS
    Case("s60_h2048_l2_d2_tanh", 60, 2, 2048, 2, False, True, 16, (1, 8, 9)),
    # 8 rows of 2052 floats do not fit: B = 8 takes the batched path, B = 1 the small one
    Case("s60_h2052_l2_d2", 60, 2, 2052, 2, False, False, 16, (1, 8, 9)),
    # LayerNorm with one hidden layer of ragged width; wide policy output
    Case("s17_h30_l1_d65_ln_tanh", 17, 65, 30, 1, True, True, 72, (7, 9, 64)),
    # max_batch equal to the largest batch; hidden = 64: hidden layers on l0_fwd_kernel too
    Case("s60_h64_l3_d1", 60, 1, 64, 3, False, False, 65, (1, 9, 64, 65)),
    Case("s3_h132_l3_d70_tanh", 3, 70, 132, 3, False, True, 72, (2, 9, 63)),
    Case("s68_h260_l1_d64_ln", 68, 64, 260, 1, True, False, 72, (1, 9, 65)),
    Case("s1_h30_l3_d2_ln_tanh", 1, 2, 30, 3, True, True, 72, (2, 7, 9, 63)),
]
BY_NAME = {c.name: c for c in CASES}
ALLOWED_BATCHES = (1, 2, 7, 8, 9, 63, 64, 65, 130)
X_ROWS = max(ALLOWED_BATCHES)

# ---- the host code's choice of launches (iql_api.inc), restated --------------------------------------------------
SMALL_FWD_MAX_B = 8                    # kernels.hpp
SMALL_FWD_LDS_BYTES = 64 * 1024        # iql_api.inc: B x K floats of a layer's input are staged in LDS
L0_KP, SKN_T = 64, 64                  # l0_fwd.hpp, skinny.hpp
SMALL, L0, SKINNY, GEMM, LN = ("small_fwd_kernel", "l0_fwd_kernel", "mean_skinny_kernel", "gemm_f32_kernel",
                               "ln_relu_fwd_kernel")
LABELLED = (SMALL, L0, SKINNY, GEMM)   # launches the profiler names (every grouped-GEMM label starts with GEMM)


def small_path(case, B, which):
    """`which`: "vf", "v_target" or "policy".  The policy net never has LayerNorm."""
    fits = 4 * B * max(case.S, case.H) <= SMALL_FWD_LDS_BYTES
    return B <= SMALL_FWD_MAX_B and fits and not (which != "policy" and case.layer_norm)


def _l0_ok(case, K, ln, fused_head):
    return 4 <= K <= L0_KP and K % 4 == 0 and case.H % 4 == 0 and not ln and not fused_head


def expected_kernels(case, B, which):
    """[(role, kernel)] in launch order.  Roles: "input" (layer 0), "hidden" (a later hidden layer), "ln" (LayerNorm +
    ReLU of the layer before it), "head" (value output), "mean" (policy output), "pack" / "finish" (unlabelled)."""
    S, H, L, D = case.S, case.H, case.L, case.D
    value = which != "policy"
    if small_path(case, B, which):
        return [("input" if l == 0 else "hidden", SMALL) for l in range(L)] + [("head" if value else "mean", SMALL)]
    out = [("pack", "pack_kernel")]
    ln = value and case.layer_norm
    for l in range(L):
        K = S if l == 0 else H
        # the value nets' last hidden layer is never stored without LayerNorm: its head is the product's epilogue
        fused = value and l == L - 1 and not ln
        out.append(("input" if l == 0 else "hidden", L0 if _l0_ok(case, K, ln, fused) else GEMM))
        if ln:
            out.append(("ln", LN))
    if value:
        out.append(("finish", "head_finish_kernel"))
    else:
        out.append(("mean", SKINNY if D <= SKN_T and H % 4 == 0 else GEMM))
        out.append(("finish", "mean_finish_kernel"))
    return out


def labelled_counts(case, B, which):
    """{kernel: launches} of the launches the profiler names."""
    out = {}
    for _, k in expected_kernels(case, B, which):
        if k in LABELLED:
            out[k] = out.get(k, 0) + 1
    return out


# ---- parameters and inputs -------------------------------------------------------------------------------------------
def _net(rng, dims, ln):
    """One MLP: weights ~ sqrt(2 / fan_in) (activations stay O(1) through ReLU), every bias and affine term non-zero."""
    L = len(dims) - 2
    f = lambda a: np.ascontiguousarray(a, np.float32)
    away = lambda shape, lo, hi: rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)     # |v| in [lo, hi]
    return dict(
        w=[f(rng.standard_normal((dims[l + 1], dims[l])) * np.sqrt((2.0 if l else 1.0) / dims[l])) for l in range(L + 1)],
        b=[f(away(dims[l + 1], 0.05, 0.4)) for l in range(L + 1)],
        lnw=[f(rng.uniform(0.7, 1.3, dims[l + 1])) for l in range(L)] if ln else [],
        lnb=[f(away(dims[l + 1], 0.05, 0.3)) for l in range(L)] if ln else [])


def fill(case, seed=0):
    """numpy parameters of the five networks: {"vf": [v1, v2], "v_target": [v1, v2], "policy": net, "log_std": (D,)},
    a net being {"w": [L+1], "b": [L+1], "lnw": [L], "lnb": [L]}.  The target twin is drawn on its own."""
    rng = np.random.default_rng([seed, case.S, case.D, case.H, case.L, int(case.layer_norm)])
    vdims = [case.S] + [case.H] * case.L + [1]
    pdims = [case.S] + [case.H] * case.L + [case.D]
    arrays = {"vf": [_net(rng, vdims, case.layer_norm) for _ in range(2)],
              "v_target": [_net(rng, vdims, case.layer_norm) for _ in range(2)],
              "policy": _net(rng, pdims, False),
              "log_std": np.float32(rng.uniform(0.1, 0.5, case.D) * rng.choice([-1.0, 1.0], case.D))}
    for twin in ("vf", "v_target"):            # a head bias that is plainly visible in the value
        for i, net in enumerate(arrays[twin]):
            net["b"][case.L][:] = np.float32((0.75 + 0.25 * i) * (-1.0 if twin == "vf" else 1.0))
    return arrays


def _net_tensors(net, L):
    out = []
    for l in range(L + 1):
        out += [net["w"][l], net["b"][l]]
        if net["lnw"] and l < L:
            out += [net["lnw"][l], net["lnb"][l]]
    return out


def group_tensors(case, arrays, group):
    """The arrays of one flat arena in the engine's tensor_table order: "vf" / "v_target" (both twins) or "policy"
    (log_std first).  A weight is (out, in), everything else 1-D."""
    if group == "policy":
        return [arrays["log_std"]] + _net_tensors(arrays["policy"], case.L)
    return _net_tensors(arrays[group][0], case.L) + _net_tensors(arrays[group][1], case.L)


def oracle_params(case, arrays):
    """The state dict oracle.por_oracle.mlp_forward / twin_forward read: prefixes vf, v_target, goal_policy.net."""
    P = {"goal_policy.log_std": arrays["log_std"]}
    for twin in ("vf", "v_target"):
        P.update(zip(O.twin_param_names(twin, case.L, case.layer_norm), group_tensors(case, arrays, twin)))
    P.update(zip(O.mlp_param_names("goal_policy.net", case.L, False), _net_tensors(arrays["policy"], case.L)))
    return P


def inputs(case, seed=0):
    """(X_ROWS, S) float32; a batch of B rows is its first B rows, so the 8-row and the 9-row call share rows.  Every
    fifth column from 1 is exactly zero, every fifth from 3 is negative throughout."""
    rng = np.random.default_rng([seed + 1000, case.S])
    x = rng.standard_normal((X_ROWS, case.S))
    x[:, 1::5] = 0.0
    x[:, 3::5] = -np.abs(x[:, 3::5]) - 0.01
    return np.ascontiguousarray(x, np.float32)


# ---- reference and bar -----------------------------------------------------------------------------------------------
BAR_FLOOR, BAR_FACTOR = 2e-6, 4.0
OUTPUTS = ("vf1", "vf2", "tgt1", "tgt2", "mean")


def error(got, ref64):
    """max |got - ref64| / max(1, max |ref64|)"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    return float(np.abs(got - ref64).max() / max(1.0, np.abs(ref64).max()))


def oracle_outputs(case, P, x, dtype):
    """The five outputs of the forward entry points by the numpy oracle at working precision `dtype`."""
    O.set_precision(dtype)
    try:
        Pd = {k: np.asarray(v, dtype) for k, v in P.items()}
        xd = np.asarray(x, dtype)
        v1, v2, _, _ = O.twin_forward(Pd, "vf", xd, case.L, case.layer_norm)
        t1, t2, _, _ = O.twin_forward(Pd, "v_target", xd, case.L, case.layer_norm)
        mean, _ = O.mlp_forward(Pd, "goal_policy.net", xd, case.L, False, "tanh" if case.pol_tanh else None)
    finally:
        O.set_precision(np.float32)
    return dict(zip(OUTPUTS, (v1, v2, t1, t2, mean)))


@lru_cache(maxsize=None)
def case_data(name, seed=0):
    case = BY_NAME[name]
    arrays = fill(case, seed)
    return case, arrays, oracle_params(case, arrays), inputs(case, seed)


def reference_for(case, P, x):
    """-> {"ref": {output: fp64 array}, "e32": {output: error of the fp32 oracle}, "bar": {output: limit}} for the
    parameters `P` (oracle_params keys) and rows `x`.  The bar is max(2e-6, 4 x e32): 2e-6 is what the engine's forward
    tests hold at hidden <= 256; the factor covers three fp32 summation orders that owe each other no rounding (MFMA
    k-order, the lane-strided GEMV with its shuffle tree, the CPU BLAS)."""
    ref = oracle_outputs(case, P, x, np.float64)
    o32 = oracle_outputs(case, P, x, np.float32)
    for v in ref.values():
        v.setflags(write=False)
    e32 = {k: error(o32[k], ref[k]) for k in OUTPUTS}
    return {"ref": ref, "e32": e32, "bar": {k: max(BAR_FLOOR, BAR_FACTOR * e32[k]) for k in OUTPUTS}}


@lru_cache(maxsize=None)
def reference(name, B, seed=0):
    """`reference_for` the first B input rows of case `name`: computed once, shared by the tests, read-only."""
    case, _, P, x = case_data(name, seed)
    return reference_for(case, P, x[:B])
