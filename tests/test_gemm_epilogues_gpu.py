"""The grouped fp32 GEMM's operand prologue and every epilogue of GemmProb (csrc/gemm_f32.hpp), launched descriptor by
descriptor through porl_gemm_f32_group and pinned PER ELEMENT to the fp64 reference of tests/helpers/gemm_cases.py.

Exact cases hold small integers, so the comparison is np.array_equal (tests/test_gemm_cases.py proves on the CPU that
nothing leaves the fp32 significand); rounded cases carry a bound derived from the operation count.  Every output
buffer is larger than its defined region and prefilled with a sentinel that must survive outside the region.  GPU only."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import gemm_cases as GC
from porl_amd import _native as N
from porl_amd.engine import gemm_f32_group

DEV = "cuda"
TILES = GC.ALL_TILES
# (tile, single_buffer) the operand prologue is instantiated for
APRO_CONFIGS = [(1, 0), (3, 0), (4, 0), (3, 1)]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _upload(d):
    """Device tensors of one case: (porl_gemm_desc fields for engine.gemm_f32_group, the output tensors by name)."""
    outs = {k: _dev(v) for k, v in GC.init_outputs(d).items()}
    desc = dict(mode=d.mode, M=d.M, N=d.N, K=d.K, lda=d.lda, ldb=d.ldb, ldc=d.ldc, ldmask=d.ldmask, act=d.act,
                A=_dev(d.A), B=_dev(d.B), C=outs["C"], bias=_dev(d.bias), mask=_dev(d.mask), headw=_dev(d.headw),
                headout=outs.get("headout"), colsum=outs.get("colsum"), cstat=outs.get("cstat"),
                a_colscale=_dev(d.colscale), a_colshift=_dev(d.colshift),
                resid=None if d.resid is None else outs["C" if d.resid_kind == "alias" else "resid"],
                rscale=_dev(d.rscale), rs_rows=d.rs_rows, rs_row0=d.rs_row0, a_grp=d.a_grp, a_grp_jump=d.a_grp_jump,
                a_seg_tiles=d.a_seg_tiles, a_seg_jump=d.a_seg_jump, splitk=d.splitk, store_c=d.store_c)
    return desc, outs


def _case(c):
    return GC.CASES[c] if isinstance(c, str) else c          # a name from the table, or a Desc made on the spot


def _launch(names, tile, single_buffer=0):
    """ONE launch of the named cases as one group; the output buffers afterwards, as numpy, one dict per case."""
    up = [_upload(_case(n)) for n in names]
    gemm_f32_group([u[0] for u in up], tile=tile, single_buffer=single_buffer)
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in u[1].items()} for u in up]


def _run_and_check(name, tile, single_buffer=0):
    got = _launch([name], tile, single_buffer)[0]
    GC.check_outputs(GC.CASES[name], GC.ref(name), got, what=f"tile {tile} single_buffer {single_buffer}")
    return got


def _refused(names, tile, single_buffer=0, code=None):
    """The launch must come back as PORL_ERR_INVALID / PORL_ERR_UNSUPPORTED and leave every output at its initial image."""
    cases = [_case(n) for n in names]
    up = [_upload(d) for d in cases]
    with pytest.raises(N.NativeError, match=r"rc=-[12]\)" if code is None else rf"rc={code}\)"):
        gemm_f32_group([u[0] for u in up], tile=tile, single_buffer=single_buffer)
    torch.cuda.synchronize()
    for d, (_, outs) in zip(cases, up):
        for k, v in GC.init_outputs(d).items():
            assert np.array_equal(outs[k].cpu().numpy(), v), f"{d.name}: {k} touched by a refused call"


# ---- 1-5, K = 0: one feature at a time, every tile ----------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", GC.names("head"))
def test_fused_head(name, tile):
    # headout[p, m] = sum over the 32 columns of part p of the stored C * headw, also where N % 32 != 0 and with
    # store_c = 0 (C keeps its sentinel)
    _run_and_check(name, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", GC.names("colsum"))
def test_column_sums(name, tile):
    _run_and_check(name, tile)         # only the tn == 0 column of blocks writes; N spans several column tiles


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", GC.names("splitk"))
def test_split_k_slabs(name, tile):
    _run_and_check(name, tile)         # C slabs and colsum slabs compared slab by slab; empty splits give zeros


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", GC.names("resid"))
def test_residual_form(name, tile):
    _run_and_check(name, tile)         # rs_rows = 7, rs_row0 = 3: sample boundaries inside and across tiles


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", GC.names("cstat"))
def test_column_statistics(name, tile):
    _run_and_check(name, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", GC.names("mask"))
def test_mask(name, tile):
    _run_and_check(name, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", GC.names("k0"))
def test_k_zero_stores_the_activated_bias(name, tile):
    d = GC.CASES[name]
    got = _run_and_check(name, tile)
    want = np.maximum(d.bias, 0) if d.act == GC.ACT_RELU else d.bias
    assert np.array_equal(got["C"][:d.M, :d.N], np.broadcast_to(want, (d.M, d.N)))


def test_auto_tile():
    for name in ("head_s1_k160", "colsum_s2_k100", "resid_s3_k32_rs_sep"):
        _run_and_check(name, -1)


# ---- 6: the BN + ReLU operand prologue -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,single_buffer", APRO_CONFIGS)
@pytest.mark.parametrize("name", GC.names("apro"))
def test_operand_prologue(name, tile, single_buffer):
    _run_and_check(name, tile, single_buffer)


def test_operand_prologue_refusals():
    _refused(["apro_s1_k32"], 0)
    _refused(["apro_s1_k32"], 2)
    for bad in (GC.make("apro_k100", GC.NT, 200, 136, 100, 1, apro=True),
                GC.make("apro_nn", GC.NN, 200, 136, 96, 2, apro=True),
                GC.make("apro_tn", GC.TN, 200, 136, 96, 3, apro=True),
                GC.make("apro_unaligned", GC.NT, 100, 70, 96, 4, apro=True, ldc=73, lda_pad=1, ldb_pad=3)):
        for tile in GC.APRO_TILES:
            _refused([bad], tile)
    _refused(["apro_s1_k32", "cstat_s1_k128"], 3)           # a group shares the prologue


# ---- 7: the single-buffer schedule without the prologue ------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.names("onebuf") + ["gather_n72", "head_s1_k160", "resid_s1_k96_rs_alias"])
def test_single_buffer(name):
    got = _run_and_check(name, 3, single_buffer=1)
    two = _launch([name], 3, 0)[0]                            # the same arithmetic on the double-buffered schedule
    assert all(np.array_equal(got[k], two[k]) for k in got)


# ---- 8: A gathered from 2x2 patches of an NHWC tensor ------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", GC.names("gather"))
def test_gathered_patch_operand(name, tile):
    _run_and_check(name, tile)


# ---- 9: groups ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("family", ["group4", "group4v", "group8"])
def test_groups(family, tile):
    # group4 holds one problem with odd leading dimensions, which puts the WHOLE group on the dword-load kernel;
    # group4v is readable with 16-byte loads throughout; group8 fills the group and mixes in split-K and K = 0
    names = GC.names(family)
    grouped = _launch(names, tile)
    for n, g in zip(names, grouped):
        GC.check_outputs(GC.CASES[n], GC.ref(n), g, what=f"in {family}, tile {tile}")
        alone = _launch([n], tile)[0]
        assert all(np.array_equal(g[k], alone[k]) for k in g), f"{n}: grouped and single launches differ"


@pytest.mark.parametrize("tile", TILES)
def test_rounded_group_is_bit_identical_to_single_launches(tile):
    # with rounded operands bit-identity is not implied by the reference: a problem's blocks must do the same
    # arithmetic wherever the group places them
    names = ["r_head", "r_mask", "r_splitk3", "r_cstat", "r_resid"]
    for n, g in zip(names, _launch(names, tile)):
        GC.check_outputs(GC.CASES[n], GC.ref(n), g, what=f"in a rounded group, tile {tile}")
        alone = _launch([n], tile)[0]
        assert all(np.array_equal(g[k], alone[k]) for k in g), f"{n}: grouped and single launches differ"


def test_group_size_limits():
    _refused(GC.names("group8") + ["k0_s2_bias"], 3, code=-1)        # nprob = 9
    with pytest.raises(N.NativeError, match=r"rc=-1\)"):
        gemm_f32_group([], tile=3)
    _refused(["head_s1_k160"], 5, code=-1)
    _refused(["head_s1_k160"], -2, code=-1)


# ---- 10: mask / resid together with cstat / head ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GC.names("combo"))
def test_mask_or_resid_with_stats_or_head_is_refused(name):
    """cstat and the head are defined on the STORED C.  Interior 16-byte tiles apply mask / resid in their final store
    loop, after both were taken; edge tiles apply them before.  On (200, 136) both kinds of tile occur.  No engine
    combines them, so the launch refuses instead of computing two definitions in one product."""
    for tile in TILES:
        _refused([name], tile, code=-2)


# ---- rounded cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", GC.names("rounded"))
def test_rounded(name, tile):
    _run_and_check(name, tile)


@pytest.mark.parametrize("tile,single_buffer", APRO_CONFIGS)
def test_rounded_operand_prologue(tile, single_buffer):
    _run_and_check("r_apro", tile, single_buffer)


# ---- host refusals of the entry that need device pointers to be told from a launch ------------------------------------------------------
def test_refused_descriptors_launch_nothing():
    d = GC.make("bad", GC.TN, 64, 64, 64, 9, colsum=True, splitk=2)
    d.mode = GC.NT                                           # colsum with a k-contiguous A: the kernel would ignore it
    d.A, d.lda = d.A.T.copy(), 64
    _refused([d], 3, code=-1)
    d.mode, d.bias = GC.TN, np.zeros(64, np.float32)         # splitk with an epilogue the raw slab path drops
    _refused([d], 3, code=-2)
    d = GC.make("short_ldc", GC.NT, 64, 64, 64, 10)          # extents: rows of C / of the mask would overlap
    d.ldc = 60
    _refused([d], 3, code=-1)
    d = GC.make("short_ldmask", GC.NT, 64, 64, 64, 11, mask=True)
    d.ldmask = 60
    _refused([d], 3, code=-1)
    d = GC.make_gathered("odd_jump", 906)                    # a jump that would move 16-byte loads off their alignment
    d.a_seg_jump += 2
    _refused([d], 3, code=-1)
