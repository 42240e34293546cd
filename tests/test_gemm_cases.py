"""CPU-side conditions of tests/test_gemm_epilogues_gpu.py: the exact cases ARE exact in fp32, and the fp64 reference
(tests/helpers/gemm_cases.py) computes what it says, checked on hand-made inputs and against plain numpy."""
import numpy as np
import pytest

from helpers import gemm_cases as GC

EXACT = [n for n, d in GC.CASES.items() if d.exact]


@pytest.mark.parametrize("name", EXACT)
def test_exact_cases_stay_inside_the_fp32_significand(name):
    # the table's own seed and 7 more draws of the same case: "exact in any summation order" is a condition on the
    # sum of ABSOLUTE values of every intermediate (in units of its finest step), not a hope
    d = GC.CASES[name]
    assert GC.ref(name).max_intermediate < 2 ** 24
    if d.a_grp:
        others = [GC.make_gathered(name, 5000 + s, N=d.N) for s in range(7)]
    else:
        kw = dict(ldc=d.ldc, bias=d.bias is not None, act=d.act, mask=d.mask is not None, ldmask=d.ldmask or None,
                  head=d.want_head, colsum=d.want_colsum, resid=d.resid_kind, rscale=d.rscale is not None, cstat=d.want_cstat, apro=d.colscale is not None,
                  splitk=d.splitk)
        others = [GC.make(name, d.mode, d.M, d.N, d.K, 5000 + s, **kw) for s in range(7)]
    for o in others:
        assert GC.reference(o).max_intermediate < 2 ** 24
    for o in [d] + others:             # the operand ranges the bound was reasoned for
        for op in (o.A, o.B):
            assert np.abs(op[op != GC.POISON]).max(initial=0) <= 2
        for arr, lim in ((o.bias, 3), (o.headw, 3), (o.resid, 8), (o.colshift, 2)):
            assert arr is None or (np.abs(arr).max() <= lim and np.array_equal(arr, np.round(arr)))
        assert o.rscale is None or set(np.unique(o.rscale)) <= {0.0, 0.5, 1.0, 2.0}
        assert o.colscale is None or set(np.unique(o.colscale)) <= {1.0, 2.0}
        assert o.K <= 160


def test_every_issue_shape_and_k_is_in_the_table():
    shapes = {(d.M, d.N, d.ldc) for d in GC.CASES.values()}
    assert {(200, 136, 136), (100, 70, 73), (1, 5, 5)} <= shapes
    assert {0, 32, 96, 100, 128, 160} <= {d.K for d in GC.CASES.values()}
    s2 = [d for d in GC.CASES.values() if (d.M, d.N, d.ldc) == (100, 70, 73)]
    assert all(d.lda % 2 == 1 and d.ldb % 2 == 1 for d in s2) and any(d.ldmask % 2 == 1 for d in s2 if d.mask is not None)
    assert GC.k_ranges(100, 7) == [(0, 32), (32, 64), (64, 96), (96, 100), (100, 100), (100, 100), (100, 100)]
    assert GC.k_ranges(160, 2) == [(0, 96), (96, 160)] and GC.k_ranges(96, 1) == [(0, 96)]


def test_gathered_operand_is_space_to_depth():
    for d in (GC.CASES["gather_n72"], GC.CASES["r_gather"]):
        assert np.array_equal(GC.gather_rows(d), d.A_dense)
        assert (d.lda, d.a_grp, d.a_grp_jump, d.a_seg_tiles, d.a_seg_jump, d.M, d.K) == (32, 5, 160, 1, 128, 100, 64)


def test_reference_on_hand_made_inputs():
    # 2 x 3 x 2 by hand: A = [[1, 2], [3, -1]], B (N, K) = [[1, 0], [0, 1], [1, 1]] -> acc = [[1, 2, 3], [3, -1, 2]]
    d = GC.make("hand", GC.NT, 2, 3, 2, 0, bias=True, act=GC.ACT_RELU, head=True, cstat=True)
    d.A[:, :2] = [[1, 2], [3, -1]]
    d.B[:, :2] = [[1, 0], [0, 1], [1, 1]]
    d.bias[:] = [0, -1, 1]
    d.headw[:] = [1, 2, -1]
    r = GC.reference(d)                                  # v = relu([[1, 1, 4], [3, -2, 3]]) = [[1, 1, 4], [3, 0, 3]]
    assert np.array_equal(r.C[0], [[1, 1, 4], [3, 0, 3]])
    assert np.array_equal(r.cstat, [[[4, 1, 7], [10, 1, 25]]])
    assert np.array_equal(r.head, [[1 + 2 - 4, 3 + 0 - 3]])
    # mask, then the residual form with the sample scale looked up at (row + rs_row0) // rs_rows
    d = GC.make("hand2", GC.NN, 2, 3, 2, 0, mask=True, resid="sep", rscale=True, rs_rows=2, rs_row0=1)
    d.A[:, :2] = [[1, 2], [3, -1]]
    d.B[:, :3] = [[1, 0, 1], [0, 1, 1]]
    d.mask[:, :3] = [[1, -1, 0], [0.5, 2, -3]]
    d.resid[:] = [[10, 20, 30], [40, 50, 60]]
    d.rscale = np.float32([2, 0.5])                      # row 0 -> index 0, row 1 -> index 1
    r = GC.reference(d)
    assert np.array_equal(r.C[0], [[10 + 2 * 1, 20, 30], [40 + 0.5 * 3, 50 - 0.5, 60]])
    # TN column sums per split, and an empty split
    d = GC.make("hand3", GC.TN, 3, 2, 40, 0, colsum=True, splitk=3)
    r = GC.reference(d)
    assert GC.k_ranges(40, 3) == [(0, 32), (32, 40), (40, 40)]
    assert np.array_equal(r.colsum[0], d.A[:32, :3].sum(0)) and np.array_equal(r.colsum[1], d.A[32:40, :3].sum(0))
    assert not r.colsum[2].any() and not r.C[2].any()
    assert np.array_equal(r.C.sum(0), d.A[:40, :3].astype(np.float64).T @ d.B[:40, :2])


def test_prologue_reference_and_bounds_are_positive():
    d = GC.CASES["apro_s1_k96_bias_cstat"]
    a = np.maximum(d.A[:, :96].astype(np.float64) * d.colscale + d.colshift, 0)
    want = a @ d.B[:, :96].astype(np.float64).T + d.bias
    assert np.array_equal(GC.ref(d.name).C[0], want)
    for name in GC.names("rounded", "rounded_apro"):
        r = GC.ref(name)
        for k in ("C_bound", "cstat_bound", "head_bound", "colsum_bound"):
            if hasattr(r, k):
                b = getattr(r, k)
                assert np.all(b >= 0) and np.all(np.isfinite(b)), (name, k)
        # an element of C: under two hundred roundings of sums of order 100, far below the O(1) values themselves
        assert r.C_bound.max() < 0.01, (name, r.C_bound.max())


def test_checker_sees_a_damaged_sentinel_and_a_wrong_value():
    d = GC.CASES["cstat_s2_k100"]
    r = GC.ref(d.name)
    got = GC.init_outputs(d)
    got["C"][:d.M, :d.N] = r.C[0]
    got["cstat"][:r.cstat.shape[0]] = r.cstat
    GC.check_outputs(d, r, got)
    for key, at in (("C", (0, d.N)), ("C", (d.M, 0)), ("cstat", (r.cstat.shape[0], 0, 0))):
        bad = {k: v.copy() for k, v in got.items()}
        bad[key][at] = 0.0
        with pytest.raises(AssertionError, match="outside its region"):
            GC.check_outputs(d, r, bad)
    bad = {k: v.copy() for k, v in got.items()}
    bad["cstat"][3, 1, 69] += 1
    with pytest.raises(AssertionError, match="differs"):
        GC.check_outputs(d, r, bad)
