"""CPU checks of tests/helpers/backward_cases.py: the grid reaches the branches it claims to reach, the inputs show what
they are there to show, the fp64 oracle agrees with finite differences, and the bar catches seeded defects.  No device."""
import numpy as np
import pytest

from helpers import backward_cases as BC
from helpers import forward_cases as FC
from oracle import por_oracle as O

RUN_IDS = [BC.run_id(r) for r in BC.RUNS]


def _runs(name):
    return [r for r in BC.RUNS if r.name == name]


def _splits(run):
    return BC.splits(BC.BY_NAME[run.name], run.B, dict(run.tune).get("dw0_slabs", BC.DW0_SLABS_DEFAULT))


# ---- the grid ----------------------------------------------------------------------------------------------------------
def test_every_forward_configuration_runs_backward_at_the_block_edges():
    assert len(set(RUN_IDS)) == len(RUN_IDS)
    for c in FC.CASES:
        want = [B for B in (BC.WIDE_BATCHES if c.H >= 2048 else BC.BATCHES) if B <= c.max_batch]
        assert [r.B for r in _runs(c.name) if not r.tune and r.max_batch == c.max_batch] == want and 9 in want, c.name
        assert BC.params(c.name)[0] == c
    Bs = {r.B for r in BC.RUNS}
    # a one-row last block of the 8-row kernels (relu_head_bwd_kernel, ln_relu_bwd_kernel) and of the 4-row ones
    assert any(B > BC.HEAD_ROWS and B % BC.HEAD_ROWS == 1 for B in Bs)
    assert any(B > BC.NLL_ROWS_PER_BLOCK and B % BC.NLL_ROWS_PER_BLOCK == 1 for B in Bs) and 1 in Bs
    # a one-row and a two-row last 64-row tile
    assert {B % BC.SKN_T for B in Bs if B > BC.SKN_T} >= {1, 2}
    ln = [c for c in FC.CASES if c.layer_norm]
    assert {260, 2048} <= {c.H for c in ln} and any(c.H % 4 for c in FC.CASES)
    assert {c.L for c in FC.CASES} == {1, 2, 3}


def test_skn_split_is_the_host_codes():
    assert BC.skn_split(17, 16) == (9, 2) and BC.skn_split(3, 1) == (1, 3) and BC.skn_split(3, 2) == (2, 2)
    assert BC.skn_split(10, 8) == (5, 2) and BC.skn_split(33, 16) == (11, 3) and BC.skn_split(1, 16) == (1, 1)
    assert BC.skn_split(32, 16) == (16, 2) and BC.skn_split(17, 8) == (6, 3)
    for tiles in range(1, 70):
        for cap in (1, 2, 8, 16):
            nslab, per = BC.skn_split(tiles, cap)
            assert nslab <= cap and (nslab - 1) * per < tiles <= nslab * per


def test_the_grid_reaches_every_tile_walk_and_loop_trip():
    big, = [r for r in _runs("s60_h48_l2_d2") if r.B == BC.BIG]
    s = _splits(big)
    assert s["row_tiles"] == 17 and s["outbwd"] == (9, 2) and s["wgrad"] == (9, 2)
    assert BC.short_last_slab(17, s["outbwd"]) and BC.short_last_slab(17, s["wgrad"])       # the b0 >= B break
    one, two = [_splits(r) for r in _runs("s60_h48_l2_d2") if r.tune]
    assert one["row_tiles"] == 3 and one["wgrad"] == (1, 3) and two["wgrad"] == (2, 2)
    assert BC.short_last_slab(3, two["wgrad"]) and not BC.short_last_slab(3, one["wgrad"])
    h580, = _runs("s60_h580_l1_d6")
    s = _splits(h580)
    assert s["row_tiles"] >= 16 and s["k_tiles"] == 10 and s["mean"] == (5, 2)
    h1028, = _runs("s60_h1028_l1_d2")
    s = _splits(h1028)
    assert s["k_tiles"] == 17 and s["mean"] == (9, 2) and BC.short_last_slab(17, s["mean"])  # the k0 >= H break
    for r in _runs("s60_h2052_l2_d2"):
        s = _splits(r)
        assert s["k_tiles"] == 33 and s["mean"] == (11, 3) and s["parts"] == 65 and s["head_passes"] >= 2
        assert s["nll_general"] and s["ncl"] == 1 and s["mean"][0] <= BC.NLL_FAST_SLABS       # general through parts only
    reasons = set()
    for r in BC.RUNS:
        s, ok = _splits(r), BC.qualifies(BC.BY_NAME[r.name])
        nslab = s["mean"][0] if ok[BC.MEAN] else None
        reasons |= {"ncl"} if s["ncl"] > 1 else set()
        reasons |= {"parts"} if s["parts"] > 64 else set()
        reasons |= {"fast"} if s["ncl"] == 1 and s["parts"] <= 64 and nslab is not None and nslab <= 16 else set()
    assert reasons == {"ncl", "parts", "fast"}
    for r in big, h580, h1028:
        assert all(BC.qualifies(BC.BY_NAME[r.name]).values()) and not BC.BY_NAME[r.name].layer_norm


def test_the_skinny_conditions_split_the_grid():
    q = {c.name: BC.qualifies(c) for c in BC.CASES}
    for k in BC.SKINNY_KERNELS:
        assert {v[k] for v in q.values()} == {True, False}, k
    c = BC.BY_NAME["s60_h48_l2_d2"]
    assert BC.skinny_kernels(c, "value") == {BC.WGRAD: 1}
    assert BC.skinny_kernels(c, "policy") == {BC.WGRAD: 1, BC.MEAN: 1, BC.OUTBWD: 1}
    assert BC.skinny_kernels(c, "policy", 1) == BC.skinny_kernels(c, "policy", 7)           # 1 reads as "all"
    assert BC.skinny_kernels(c, "policy", 2) == {BC.MEAN: 1} and BC.skinny_kernels(c, "policy", 4) == {BC.OUTBWD: 1}
    assert BC.skinny_kernels(c, "forward") == {BC.MEAN: 1}
    assert BC.skinny_kernels(c, "gradient") == {BC.WGRAD: 1, BC.OUTBWD: 1}
    assert BC.skinny_kernels(c, "policy", 0) == {} == BC.skinny_kernels(c, "value", 6)
    ln = BC.BY_NAME["s17_h48_l3_d6_ln"]
    assert BC.skinny_kernels(ln, "value") == {} and BC.skinny_kernels(ln, "policy")[BC.WGRAD] == 1
    assert BC.skinny_kernels(BC.BY_NAME["s68_h132_l1_d65"], "policy") == {}                 # S = 68, D = 65
    assert BC.skinny_kernels(BC.BY_NAME["s3_h30_l2_d6_tanh"], "policy") == {}               # H % 4
    wide = BC.BY_NAME["s60_h2052_l2_d2"]
    assert BC.skinny_kernels(wide, "policy", short_blocks=True) == {} != BC.skinny_kernels(wide, "policy")


# ---- the inputs --------------------------------------------------------------------------------------------------------
def test_log_std_holds_the_four_clamp_cases():
    seen = set()
    for c in BC.CASES:
        ls = BC.params(c.name)[2]["goal_policy.log_std"]
        assert ls.dtype == np.float32 and ls.shape == (c.D,)
        kinds = {"below": (ls < -5).any(), "above": (ls > 2).any(), "low": (ls == np.float32(-5.0)).any(),
                 "high": (ls == np.float32(2.0)).any()}
        if c.D >= 4:
            assert all(kinds.values()), c.name
            if c.D > 4:
                assert ((ls > -5) & (ls < 2)).sum() == c.D - 4
        else:
            assert sum(kinds.values()) == c.D, c.name
            seen |= {(c.D, k) for k, v in kinds.items() if v}
        assert len(BC.clamped_out(c.name)) == int(kinds["below"]) + int(kinds["above"])
        # the output units of the columns with sigma = e^-5 are forward_cases.fill's times 2^-8, the others untouched
        plain, mine = FC.fill(c)["policy"], BC.params(c.name)[1]["policy"]
        scale = np.where(ls <= -5, np.float32(2.0 ** -8), np.float32(1.0))
        assert np.array_equal(mine["w"][c.L], plain["w"][c.L] * scale[:, None])
        assert np.array_equal(mine["b"][c.L], plain["b"][c.L] * scale)
        assert all(np.array_equal(a, b) for l in range(c.L) for a, b in zip((mine["w"][l], mine["b"][l]), (plain["w"][l], plain["b"][l])))
    assert seen == {(D, k) for D in (1, 2) for k in ("below", "above", "low", "high")} - {(1, "below"), (1, "high")}


@pytest.mark.parametrize("name", [c.name for c in BC.CASES])
def test_the_pool_yields_the_largest_batch_of_decided_rows(name):
    case, _, P = BC.params(name)
    pool = BC.pool(name)
    B = BC.max_batch_of(name)
    assert pool["n_decided"] >= B and pool["n_pool"] == BC.pool_size(name)
    obs = BC.batch(name, B)[0]
    O.set_precision(np.float64)
    try:
        P64 = {k: v.astype(np.float64) for k, v in P.items()}
        for prefix, ln in (("vf.v1", case.layer_norm), ("vf.v2", case.layer_norm), ("goal_policy.net", False)):
            zs = BC._preacts(P64, prefix, obs.astype(np.float64), case.L, ln)
            assert len(zs) == case.L and min(np.abs(z).min() for z in zs) >= BC.MARGIN, prefix
    finally:
        O.set_precision(np.float32)
    assert set(np.unique(pool["term"])) == {0.0, 1.0} and (pool["rew"] > 0).any() and (pool["rew"] < 0).any()
    assert np.abs(pool["rew"]).max() < 5


@pytest.mark.parametrize("rid", RUN_IDS)
def test_every_batch_shows_the_clip_and_both_signs(rid):
    run = BC.RUNS[RUN_IDS.index(rid)]
    for mode in BC.WEIGHT_MODES:
        ref = BC.backward64(run.name, run.B, mode)
        assert np.isfinite(ref["stats"]).all()
        if run.B < 9:
            continue
        clipped = ref["raw_weight"] > O.EXP_ADV_MAX
        assert clipped.any() and not clipped.all(), rid
        assert (ref["weight"][clipped] == O.EXP_ADV_MAX).all() and (ref["weight"][~clipped] < O.EXP_ADV_MAX).all()
        for u in ref["u"]:
            assert (u < 0).any() and (u > 0).any(), rid
        _, _, _, term, _ = BC.batch(run.name, run.B)
        assert 0 < term.sum() < run.B


def test_clamped_out_log_std_has_an_exactly_zero_gradient_and_the_ends_do_not():
    for name in ("s17_h48_l3_d6_ln", "s64_h132_l2_d64_tanh", "s1_h48_l1_d1_tanh", "s60_h64_l3_d1"):
        ls = BC.params(name)[2]["goal_policy.log_std"]
        for fn in (BC.backward64, BC.backward32):
            g = fn(name, 9, 0)["grads"]["goal_policy.log_std"]
            assert (g[BC.clamped_out(name)] == 0).all()
            ends = np.flatnonzero((ls == np.float32(-5.0)) | (ls == np.float32(2.0)))
            assert (g[ends] != 0).all()
    # D = 1 with its entry above 2: the whole tensor's reference is zero, so only exact zeros pass
    assert not BC.backward64("s1_h48_l1_d1_tanh", 9, 0)["grads"]["goal_policy.log_std"].any()
    assert BC.tensor_error(np.zeros(1), np.zeros(1)) == 0.0 and BC.tensor_error(np.full(1, 1e-30), np.zeros(1)) == np.inf


# ---- the oracle against finite differences ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,mode", [("s3_h30_l2_d6_tanh", 9, 0), ("s17_h48_l3_d6_ln", 9, 1), ("s60_h48_l2_d2", 9, 1)])
def test_backward64_agrees_with_central_finite_differences(name, B, mode):
    """The analytic gradients, independently of the engine: (f(p + h) - f(p - h)) / 2h in fp64 on decided rows (a step of
    1e-6 moves no pre-activation across its MARGIN), a few seeded elements of every tensor.  At log_std exactly -5.0 /
    2.0 the clamp has a kink and autograd passes the inside slope: the difference is taken one-sided, into the range."""
    case, _, P = BC.params(name)
    ref = BC.backward64(name, B, mode)
    P64 = {k: np.array(v, np.float64) for k, v in P.items()}
    rng = np.random.default_rng(5)
    h = 1e-6
    for group in (0, 1):
        for tname in BC.tensor_names(case, group):
            g = ref["grads"][tname]
            scale = np.abs(g).max()
            flat = P64[tname].reshape(-1)
            picks = range(flat.size) if tname.endswith("log_std") else rng.choice(flat.size, min(4, flat.size), replace=False)
            for i in picks:
                keep = flat[i]
                lo, hi = (0.0, 1.0) if keep == -5.0 else (-1.0, 0.0) if keep == 2.0 else (-1.0, 1.0)
                vals = []
                for step in (lo, hi):
                    flat[i] = keep + step * h
                    vals.append(BC.losses64(name, B, mode, P64)[group])
                flat[i] = keep
                fd = (vals[1] - vals[0]) / ((hi - lo) * h)
                tol = (1e-7 if hi - lo == 2.0 else 1e-4) * max(scale, 1e-12) + 1e-9
                assert abs(fd - g.reshape(-1)[i]) <= tol, (tname, i, fd, g.reshape(-1)[i], scale)


# ---- the bar has teeth ---------------------------------------------------------------------------------------------------
TEETH_RUNS = [("s60_h48_l2_d2", 130), ("s17_h48_l3_d6_ln", 65), ("s64_h132_l2_d64_tanh", 65), ("s3_h30_l2_d6_tanh", 9),
              ("s1_h48_l1_d1_tanh", 65)]


def test_the_fp32_control_is_within_its_own_bar_and_no_bar_is_wide():
    for run in BC.RUNS:
        for mode in BC.WEIGHT_MODES:
            ref = BC.reference(run.name, run.B, mode)
            assert all(np.isfinite(e) and e <= ref["bar"][k] for k, e in ref["e32"].items()), BC.run_id(run)
            assert max(ref["bar"].values()) < 1e-2, (BC.run_id(run), ref["bar"])


@pytest.mark.parametrize("defect", BC.DEFECTS)
def test_a_seeded_defect_exceeds_the_bar_tenfold(defect):
    """Each defect, applied to the numpy fp32 run, lands at 10 x the bar of some tensor or statistic, or beyond, on at
    least one case."""
    worst = 0.0
    for name, B in TEETH_RUNS:
        case = BC.BY_NAME[name]
        for mode in BC.WEIGHT_MODES:
            ref = BC.reference(name, B, mode)
            err = BC.errors(case, BC.defective32(name, B, mode, defect), ref["ref"])
            worst = max(worst, max(err[k] / ref["bar"][k] for k in err))
    print(f"{defect}: {worst:.3g} x bar")
    assert worst >= 10.0, (defect, worst)
