"""tests/helpers/forward_cases.py on the CPU: the grid of tests/test_forward_gpu.py reaches every branch of the forward-only
host code by name, `expected_kernels` names every kernel in every role it can take, and the bar the device test holds,
max(2e-6, 4 x the fp32 oracle's own error), is met by a correct fp32 implementation on exactly these parameters and
rows (the numpy fp32 oracle against the fp64 one)."""
import numpy as np
import pytest

from helpers import forward_cases as FC


def _have(**want):
    return [c for c in FC.CASES if all(getattr(c, k) == v for k, v in want.items())]


@pytest.mark.parametrize("S", [1, 3, 17, 60, 64, 68, 364])
def test_grid_has_obs_dim(S):
    assert _have(S=S), f"no case with obs_dim {S}"


@pytest.mark.parametrize("H,ln", [(30, None), (48, None), (132, None), (260, True), (2048, True), (2048, False),
                                  (2052, False)])
def test_grid_has_hidden_dim(H, ln):
    assert _have(H=H) if ln is None else _have(H=H, layer_norm=ln), f"no case with hidden_dim {H}, layer_norm {ln}"


@pytest.mark.parametrize("L", [1, 2, 3])
def test_grid_has_n_hidden(L):
    assert _have(L=L)
    assert _have(L=L, layer_norm=True) and _have(L=L, layer_norm=False)


@pytest.mark.parametrize("D", [1, 2, 6, 64, 65, 70])
def test_grid_has_policy_width(D):
    assert _have(D=D), f"no case with pol_out_dim {D}"


def test_grid_has_both_settings_of_tanh_and_layer_norm():
    for flag in (False, True):
        assert _have(pol_tanh=flag), f"no case with pol_tanh {flag}"
        assert _have(layer_norm=flag), f"no case with layer_norm {flag}"
    # tanh past the small path and past the skinny mean
    assert any(c.pol_tanh and max(c.batches) >= 9 and c.D > 64 for c in FC.CASES)
    assert any(c.pol_tanh and max(c.batches) >= 9 and c.D <= 64 and c.H % 4 == 0 for c in FC.CASES)


def test_grid_batches_and_cost():
    assert len({c.name for c in FC.CASES}) == len(FC.CASES) <= 18
    seen = set()
    for c in FC.CASES:
        assert 3 <= len(c.batches) <= 5 and set(c.batches) <= set(FC.ALLOWED_BATCHES), c.name
        assert max(c.batches) <= c.max_batch, c.name
        if c.H >= 2048:                       # the wide engines stay cheap
            assert set(c.batches) <= {1, 8, 9} and c.S <= 64, c.name
        seen |= set(c.batches)
    assert seen == set(FC.ALLOWED_BATCHES)
    above = [c for c in FC.CASES if c.max_batch > max(c.batches)]
    assert len(above) >= len(FC.CASES) - 2                      # max_batch strictly above the largest batch on most ...
    assert any(c.max_batch == max(c.batches) for c in FC.CASES)  # ... and equal to it once
    # both sides of the switch between the two kernel families in every case, and the row-tile edges somewhere
    for c in FC.CASES:
        assert min(c.batches) <= 8 and 9 in c.batches, c.name
    assert {63, 64, 65} <= seen
    # the one configuration whose 8 rows do not fit the small path, next to the widest one that does
    wide = FC.BY_NAME["s60_h2052_l2_d2"]
    assert not FC.small_path(wide, 8, "policy") and not FC.small_path(wide, 8, "vf") and FC.small_path(wide, 7, "vf")
    assert FC.small_path(FC.BY_NAME["s60_h2048_l2_d2_tanh"], 8, "vf")


def _roles():
    """{(which, role, kernel)} over the whole grid."""
    out = set()
    for c in FC.CASES:
        for B in c.batches:
            for which in ("vf", "v_target", "policy"):
                out |= {(which, role, k) for role, k in FC.expected_kernels(c, B, which)}
    return out


@pytest.mark.parametrize("which,role,kernel", [
    # small_fwd_kernel: every layer of both families
    ("vf", "input", FC.SMALL), ("vf", "hidden", FC.SMALL), ("vf", "head", FC.SMALL), ("v_target", "head", FC.SMALL),
    ("policy", "input", FC.SMALL), ("policy", "hidden", FC.SMALL), ("policy", "mean", FC.SMALL),
    # l0_fwd_kernel: input layers, and hidden layers of width <= 64
    ("vf", "input", FC.L0), ("v_target", "input", FC.L0), ("policy", "input", FC.L0),
    ("vf", "hidden", FC.L0), ("policy", "hidden", FC.L0),
    ("policy", "mean", FC.SKINNY),
    # the grouped GEMM wherever one of those does not apply
    ("vf", "input", FC.GEMM), ("vf", "hidden", FC.GEMM), ("policy", "input", FC.GEMM), ("policy", "hidden", FC.GEMM),
    ("policy", "mean", FC.GEMM),
    # LayerNorm: value nets only
    ("vf", "ln", FC.LN), ("v_target", "ln", FC.LN),
])
def test_expected_kernels_names_every_kernel_in_every_role(which, role, kernel):
    assert (which, role, kernel) in _roles()


def test_expected_kernels_follows_the_host_predicates():
    roles = _roles()
    assert not any(w == "policy" and k == FC.LN for w, _, k in roles)
    assert not any(w != "policy" and k == FC.SKINNY for w, _, k in roles)
    ek = FC.expected_kernels
    c = FC.BY_NAME["s60_h48_l2_d2"]
    assert [k for _, k in ek(c, 8, "vf")] == [FC.SMALL] * 3
    # B = 9: layer 0 stored -> l0; layer 1 is the value nets' last (head in the epilogue) -> GEMM; the policy keeps it
    assert [k for _, k in ek(c, 9, "vf")] == ["pack_kernel", FC.L0, FC.GEMM, "head_finish_kernel"]
    assert [k for _, k in ek(c, 9, "policy")] == ["pack_kernel", FC.L0, FC.L0, FC.SKINNY, "mean_finish_kernel"]
    # L = 1: the input layer is the last one, so the value nets skip l0_fwd_kernel even at a width it takes
    c = FC.BY_NAME["s64_h132_l2_d64_tanh"]._replace(L=1)
    assert [k for _, k in ek(c, 9, "vf")] == ["pack_kernel", FC.GEMM, "head_finish_kernel"]
    assert [k for _, k in ek(c, 9, "policy")] == ["pack_kernel", FC.L0, FC.SKINNY, "mean_finish_kernel"]
    # either side of the input-layer limit, and a ragged hidden width
    assert ek(FC.BY_NAME["s64_h132_l2_d64_tanh"], 9, "policy")[1] == ("input", FC.L0)
    assert ek(FC.BY_NAME["s68_h132_l1_d65"], 9, "policy")[1] == ("input", FC.GEMM)
    assert FC.labelled_counts(FC.BY_NAME["s3_h30_l2_d6_tanh"], 9, "policy") == {FC.GEMM: 3}
    # LayerNorm values never take the small path, the policy of the same engine does
    c = FC.BY_NAME["s17_h48_l3_d6_ln"]
    assert [k for _, k in ek(c, 1, "vf")] == ["pack_kernel"] + [FC.GEMM, FC.LN] * 3 + ["head_finish_kernel"]
    assert FC.labelled_counts(c, 1, "policy") == {FC.SMALL: 4}
    # 8 rows of 2052 floats: batched path, decided for the whole chain
    c = FC.BY_NAME["s60_h2052_l2_d2"]
    assert FC.labelled_counts(c, 8, "vf") == FC.labelled_counts(c, 9, "vf") == {FC.L0: 1, FC.GEMM: 1}
    assert FC.labelled_counts(c, 8, "policy") == {FC.L0: 1, FC.GEMM: 1, FC.SKINNY: 1}
    assert FC.labelled_counts(c, 1, "policy") == {FC.SMALL: 3}


@pytest.mark.parametrize("name", [c.name for c in FC.CASES])
def test_fill_makes_every_term_visible(name):
    case, arrays, P, x = FC.case_data(name)
    assert x.shape == (FC.X_ROWS, case.S) and x.dtype == np.float32
    if case.S > 3:
        assert (x[:, 1] == 0).all() and (x[:, 3] < 0).all()
    for twin in ("vf", "v_target"):
        for net in arrays[twin]:
            assert len(net["w"]) == case.L + 1 and net["w"][case.L].shape == (1, case.H)
            assert all((b != 0).all() for b in net["b"])
            if case.layer_norm:
                assert all((np.abs(g - 1) <= 0.3).all() and np.abs(g - 1).max() > 0.1 for g in net["lnw"])
                assert all((b != 0).all() for b in net["lnb"])
    assert all((b != 0).all() for b in arrays["policy"]["b"]) and (arrays["log_std"] != 0).all()
    assert not np.array_equal(arrays["vf"][0]["w"][0], arrays["v_target"][0]["w"][0])
    names = set(P)
    assert {"vf.v1.0.weight", "v_target.v2.0.bias", "goal_policy.net.0.weight", "goal_policy.log_std"} <= names
    assert all(v.dtype == np.float32 for v in P.values())
    # activations stay O(1), and the target answers differently from the online twin by far more than the bar
    r = FC.reference(name, min(case.batches))["ref"]
    for k in FC.OUTPUTS:
        assert np.isfinite(r[k]).all() and 1e-3 < np.abs(r[k]).max() < 50, (k, np.abs(r[k]).max())
    for a, b in (("vf1", "tgt1"), ("vf2", "tgt2")):
        assert FC.error(r[a], r[b]) > 1e-2
    if case.pol_tanh:
        assert np.abs(r["mean"]).max() < 1 and np.abs(np.arctanh(r["mean"])).max() > 0.2     # squashed, not saturated


@pytest.mark.parametrize("name", [c.name for c in FC.CASES])
def test_fp32_oracle_meets_the_bar(name):
    """The bar is reachable: a plain fp32 evaluation of the same formulas sits within max(2e-6, 4 x e32) of fp64 by
    construction, and e32 itself is rounding-sized — a term dropped or a row misplaced moves an output by 1e-3."""
    case = FC.BY_NAME[name]
    for B in case.batches:
        r = FC.reference(name, B)
        assert r["ref"]["vf1"].shape == (B,) and r["ref"]["mean"].shape == (B, case.D)
        for k in FC.OUTPUTS:
            print(f"{name} B={B} {k}: e32 {r['e32'][k]:.2e} bar {r['bar'][k]:.2e}")
            assert r["e32"][k] <= r["bar"][k]
            assert r["bar"][k] <= 2e-5, (k, r["bar"][k])      # still 50 times below what a real defect moves
