"""Cases and the fp64 reference of tests/test_gemm_epilogues_gpu.py: one `Desc` holds the host arrays of one
porl_gemm_desc (include/porl_hip.h), `reference` evaluates it in float64, `init_outputs` / `check_outputs` lay out the
sentinel-filled output buffers and compare them.  numpy only, importable without a GPU (tests/test_gemm_cases.py).

Exact cases hold small integers (and halves, through rscale), so every product, partial sum, square and sum of squares
is exact in fp32 in ANY summation order, provided nothing leaves the 24-bit significand: `reference` returns the
largest magnitude any intermediate can reach, in units of the finest step that occurs, and the CPU test asserts it is
below 2^24 for every exact case.  Rounded cases (standard-normal operands, tanh, non-dyadic rscale) come with a
per-element bound DERIVED from the operation count, see `reference`.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

NT, NN, TN = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
SENTINEL = 7.0          # every output buffer is prefilled with it (as tests/test_gemm_gpu.py:test_gemm_plain)
POISON = 1000.0         # leading-dimension padding of the operands: never read by a correct kernel
ALL_TILES = (0, 1, 2, 3, 4)        # 128x128, 128x64, 64x128, 64x64, 128x96
APRO_TILES = (1, 3, 4)             # the operand prologue is instantiated for these
U = 2.0 ** -24                     # fp32 unit roundoff
TANH_ERR = 2.0 ** -22              # absolute error allowed to tanhf
# extra room behind every output so that "too far" shows as a damaged sentinel instead of a stray write
PAD_ROWS, PAD_PARTS, PAD_SLABS, PAD_BLOCKS = 2, 2, 2, 4


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def _padded(x, ld):
    out = np.full((x.shape[0], ld), POISON, np.float32)
    out[:, :x.shape[1]] = x
    return out


def make(name, mode, M, N, K, seed, *, exact=True, lda_pad=0, ldb_pad=0, ldc=None, bias=False, act=ACT_NONE, mask=False,
         ldmask=None, head=False, colsum=False, resid=None, rscale=False, rs_rows=7, rs_row0=3, cstat=False, apro=False,
         splitk=1, store_c=1):
    """resid: None, "sep" (its own buffer) or "alias" (C itself).  Exact operands: A, B in [-2, 2], bias and headw in
    [-3, 3], resid in [-8, 8], rscale in {0, 0.5, 1, 2}, colscale in {1, 2}, colshift in [-2, 2]."""
    rng = np.random.default_rng(seed)
    d = SimpleNamespace(name=name, mode=mode, M=M, N=N, K=K, exact=exact, act=act, splitk=splitk, store_c=store_c,
                        rs_rows=rs_rows, rs_row0=rs_row0, a_grp=0, a_grp_jump=0, a_seg_tiles=0, a_seg_jump=0,
                        want_head=head, want_colsum=colsum, want_cstat=cstat, resid_kind=resid)
    val = (lambda lo, hi, shape: _ints(rng, lo, hi, shape)) if exact else \
          (lambda lo, hi, shape: rng.standard_normal(shape).astype(np.float32))
    sa = (M, K) if mode in (NT, NN) else (K, M)
    sb = (N, K) if mode == NT else (K, N)
    d.lda, d.ldb = max(sa[1], 4) + lda_pad, max(sb[1], 4) + ldb_pad
    d.A, d.B = _padded(val(-2, 2, sa), d.lda), _padded(val(-2, 2, sb), d.ldb)
    d.ldc = N if ldc is None else ldc
    d.bias = val(-3, 3, N) if bias else None
    d.headw = val(-3, 3, N) if head else None
    d.ldmask = (N if ldmask is None else ldmask) if mask else 0
    d.mask = _padded(rng.standard_normal((M, N)).astype(np.float32), d.ldmask) if mask else None
    d.resid = val(-8, 8, (M, N)) if resid else None
    nrs = (M - 1 + rs_row0) // rs_rows + 1
    d.rscale = None if not rscale else (rng.choice(np.float32([0, 0.5, 1, 2]), nrs) if exact
                                        else rng.uniform(0.3, 1.7, nrs).astype(np.float32))
    d.colscale = d.colshift = None
    if apro:
        d.colscale = _ints(rng, 1, 2, K) if exact else rng.uniform(0.5, 1.5, K).astype(np.float32)
        d.colshift = val(-2, 2, K)
    return d


def make_gathered(name, seed, N=72, *, exact=True):
    """The 2x2 patch rows of an NHWC tensor (5, 8, 10, 16) read in place (PatchMerging): E = 16, K = 4E = 64,
    M = 5*4*5 = 100.  Row m = (b, i, j) starts at ((b*8 + 2i)*10 + 2j)*E = m*2E + (m // 5)*(5*2E) and its second half
    (the next image row) lies 10E - 2E further.  Epilogue: bias + cstat, as the encoder's merge product."""
    rng = np.random.default_rng(seed)
    E = 16
    x = _ints(rng, -2, 2, (5, 8, 10, E)) if exact else rng.standard_normal((5, 8, 10, E)).astype(np.float32)
    d = make(name, NT, 100, N, 4 * E, seed + 1, exact=exact, bias=True, cstat=True)
    d.A = x.reshape(-1, 2 * E)                                  # the storage the kernel sees
    d.A_dense = x.reshape(5, 4, 2, 5, 2, E).transpose(0, 1, 3, 2, 4, 5).reshape(100, 4 * E)   # numpy space-to-depth
    d.lda, d.a_grp, d.a_grp_jump, d.a_seg_tiles, d.a_seg_jump = 2 * E, 5, 5 * 2 * E, 1, 10 * E - 2 * E
    return d


def gather_rows(d):
    """The gathered operand by the ADDRESS rule of the descriptor (checked against A_dense on the CPU)."""
    flat = d.A.reshape(-1)
    m = np.arange(d.M)[:, None]
    k = np.arange(d.K)[None, :]
    return flat[m * d.lda + (m // d.a_grp) * d.a_grp_jump + k + (k >= 32 * d.a_seg_tiles) * d.a_seg_jump]


def k_ranges(K, splitk):
    """K range of every split as the planner cuts it: chunks of ceil(K / splitk) rounded up to whole K-tiles of 32."""
    s = max(splitk, 1)
    kc = -(-(-(-K // s)) // 32) * 32
    return [(min(i * kc, K), min((i + 1) * kc, K)) for i in range(s)]


def reference(d):
    """Every output of descriptor `d` in float64, plus for each its error bound and `max_intermediate`.

    Bound of an output element: (n + 2) * 2^-24 * S [+ the tanhf share], with S the same expression evaluated on absolute
    values and n the number of fp32 operations that feed the element:
      C        n = K (the fma chain) + 1 with a bias + 1 with the prologue (its fma) + 2 with resid (fmul, fadd);
               through tanh S becomes L * S + |tanh x| (L = the steepest slope of tanh within the input's bound: the
               mean value theorem for the error that arrives, |tanh x| for the roundings that follow) and 2^-22 is
               added for tanhf itself
      slab     n = the length of the split's K range
      cstat    sums: n = n_C + 32, S = sum of S_C over the block; squares: c^2 doubles c's relative error and one fma
               per row follows, n = 2 * (n_C + 2) + 32, S = sum of S_C^2
      head     n = n_C + 32 (one product and the 32-column sum), S = sum of S_C * |headw|
      colsum   n = the length of the split's K range, S = sum of |A|
    """
    f8 = np.float64
    A, B = d.A.astype(f8), d.B.astype(f8)
    if d.a_grp:
        a = gather_rows(d).astype(f8)
    elif d.mode == TN:
        a = A[:d.K, :d.M].T
    else:
        a = A[:d.M, :d.K]
    a_abs, n_c = np.abs(a), d.K
    if d.colscale is not None:
        a_abs = np.abs(a) * np.abs(d.colscale.astype(f8)) + np.abs(d.colshift.astype(f8))
        a = np.maximum(a * d.colscale.astype(f8) + d.colshift.astype(f8), 0.0)
        n_c += 1
    b = B[:d.N, :d.K].T if d.mode == NT else B[:d.K, :d.N]            # (K, N)
    r = SimpleNamespace(n_c=None)
    ranges = k_ranges(d.K, d.splitk)
    if d.splitk > 1:        # raw slabs: no epilogue
        r.C = np.stack([a[:, lo:hi] @ b[lo:hi] for lo, hi in ranges])
        S = np.stack([a_abs[:, lo:hi] @ np.abs(b[lo:hi]) for lo, hi in ranges])
        r.C_bound = np.stack([(hi - lo + 2) * U * S[i] for i, (lo, hi) in enumerate(ranges)])
        lin, sq, tanh_c = [S.max()], [], 0.0
    else:
        v, S = a @ b, a_abs @ np.abs(b)
        if d.bias is not None:
            v, S, n_c = v + d.bias.astype(f8), S + np.abs(d.bias.astype(f8)), n_c + 1
        tanh_c = np.zeros_like(v)
        if d.act == ACT_RELU:
            v = np.maximum(v, 0.0)
        elif d.act == ACT_TANH:
            # |tanh(x + e) - tanh(x)| <= L |e| with L the largest slope within the input's own bound; what follows
            # rounds values of size |tanh x|
            L = 1.0 - np.tanh(np.maximum(np.abs(v) - (n_c + 2) * U * S, 0.0)) ** 2
            v = np.tanh(v)
            S, tanh_c = L * S + np.abs(v), tanh_c + TANH_ERR
        if d.mask is not None:
            keep = d.mask[:, :d.N] > 0
            v, S, tanh_c = v * keep, S * keep, tanh_c * keep
        if d.resid is not None:
            rs = np.ones(d.M) if d.rscale is None else d.rscale.astype(f8)[(np.arange(d.M) + d.rs_row0) // d.rs_rows]
            v = d.resid.astype(f8) + rs[:, None] * v
            S = np.abs(d.resid.astype(f8)) + np.abs(rs)[:, None] * S
            tanh_c, n_c = tanh_c * np.abs(rs)[:, None], n_c + 2
        r.C, r.C_bound = v[None], ((n_c + 2) * U * S + tanh_c)[None]
        lin, sq = [S.max()], []
        if d.want_cstat:
            nb = (d.M + 31) // 32
            pad = lambda x: np.concatenate([x, np.zeros((nb * 32 - d.M, d.N))]).reshape(nb, 32, d.N)
            r.cstat = np.stack([pad(v).sum(1), (pad(v) ** 2).sum(1)], axis=1)                  # (nb, 2, N)
            s1, s2 = pad(S).sum(1), (pad(S) ** 2).sum(1)
            r.cstat_bound = np.stack([(n_c + 32 + 2) * U * s1 + pad(tanh_c).sum(1),
                                      (2 * (n_c + 2) + 32 + 2) * U * s2 + (2 * pad(S) * pad(tanh_c)).sum(1)], axis=1)
            lin.append(s1.max()); sq.append(s2.max())
        if d.want_head:
            parts = (d.N + 31) // 32
            hw = d.headw.astype(f8)
            pad = lambda x: np.concatenate([x, np.zeros((d.M, parts * 32 - d.N))], axis=1).reshape(d.M, parts, 32)
            r.head = pad(v * hw).sum(2).T                                                      # (parts, M)
            sh = pad(S * np.abs(hw)).sum(2).T
            r.head_bound = (n_c + 32 + 2) * U * sh + pad(tanh_c * np.abs(hw)).sum(2).T
            lin.append(sh.max())
    if d.want_colsum:
        assert d.mode == TN
        r.colsum = np.stack([a[:, lo:hi].sum(1) for lo, hi in ranges])                        # (splits, M)
        sc = np.stack([a_abs[:, lo:hi].sum(1) for lo, hi in ranges])
        r.colsum_bound = np.stack([(hi - lo + 2) * U * sc[i] for i, (lo, hi) in enumerate(ranges)])
        lin.append(sc.max())
    # finest step of any intermediate: 1, or 1/2 when rscale holds 0.5 (squares then step by 1/4)
    step = 0.5 if d.exact and d.rscale is not None and np.any(d.rscale == 0.5) else 1.0
    r.max_intermediate = max([x / step for x in lin] + [x / step ** 2 for x in sq])
    r.n_c = n_c
    return r


def init_outputs(d):
    """Sentinel-filled host images of the output buffers, each larger than its defined region.  With resid aliasing C
    the defined region of C starts out as the residual."""
    s, nb, parts = max(d.splitk, 1), (d.M + 31) // 32, (d.N + 31) // 32
    o = {"C": np.full(((s * d.M + PAD_ROWS), d.ldc), SENTINEL, np.float32)}
    if d.resid is not None:
        o["resid"] = np.full((d.M + PAD_ROWS, d.ldc), SENTINEL, np.float32)
        o["resid"][:d.M, :d.N] = d.resid
        if d.resid_kind == "alias":
            o["C"] = o.pop("resid")
    if d.want_head:
        o["headout"] = np.full((parts + PAD_PARTS, d.M), SENTINEL, np.float32)
    if d.want_colsum:      # (room for a slab stride of ldc instead of M as well)
        o["colsum"] = np.full((s + PAD_SLABS, max(d.M, d.ldc)), SENTINEL, np.float32).reshape(-1)
    if d.want_cstat:
        o["cstat"] = np.full((nb + PAD_BLOCKS, 2, d.N), SENTINEL, np.float32)
    return o


def check_outputs(d, r, got, what=""):
    """Every defined element equals the reference (exactly, or within its derived bound); everything else in the
    buffers is still the sentinel; with store_c = 0 all of C is."""
    s, nb, parts = max(d.splitk, 1), (d.M + 31) // 32, (d.N + 31) // 32
    tag = f"{d.name} {what}"

    def region(name, buf, idx, ref, bound):
        inside = np.zeros(buf.shape, bool)
        inside[idx] = True
        assert np.all(buf[~inside] == SENTINEL), f"{tag}: {name} written outside its region at " \
                                                 f"{np.argwhere(~inside & (buf != SENTINEL))[:4].tolist()}"
        val = buf[idx].reshape(ref.shape)
        if d.exact:
            want = ref.astype(np.float32)
            assert np.array_equal(want.astype(np.float64), ref), f"{tag}: {name} reference is not an fp32 value"
            bad = val != want
            assert not bad.any(), f"{tag}: {name} differs at {np.argwhere(bad)[:4].tolist()}: got " \
                                  f"{val[bad][:4].tolist()}, want {want[bad][:4].tolist()} ({bad.sum()} of {bad.size})"
        else:
            err = np.abs(val.astype(np.float64) - ref)
            bad = ~(err <= bound)
            assert not bad.any(), f"{tag}: {name} off at {np.argwhere(bad)[:4].tolist()}: err {err[bad][:4].tolist()} " \
                                  f"bound {bound[bad][:4].tolist()} ({bad.sum()} of {bad.size})"

    C = got["C"]
    if d.store_c:
        region("C", C.reshape(-1, d.ldc), (slice(0, s * d.M), slice(0, d.N)), r.C.reshape(s * d.M, d.N),
               r.C_bound.reshape(s * d.M, d.N))
    else:
        assert np.all(C == SENTINEL), f"{tag}: C written with store_c = 0"
    if d.resid is not None and d.resid_kind == "sep":
        keep = np.full_like(got["resid"], SENTINEL)
        keep[:d.M, :d.N] = d.resid
        assert np.array_equal(got["resid"], keep), f"{tag}: the residual operand was modified"
    if d.want_head:
        region("headout", got["headout"], (slice(0, parts), slice(None)), r.head, r.head_bound)
    if not d.exact and d.store_c and d.splitk <= 1:
        # Rounded cases, second and sharper look: cstat and the head are functions of the STORED C, so against the fp64
        # sums of the device's own C only their own 32-term reductions round: (32 + 2) * 2^-24 * S.
        c = C.reshape(-1, d.ldc)[:d.M, :d.N].astype(np.float64)
        if d.want_cstat:
            blk = np.concatenate([c, np.zeros((nb * 32 - d.M, d.N))]).reshape(nb, 32, d.N)
            own = np.stack([blk.sum(1), (blk ** 2).sum(1)], axis=1)
            lim = 34 * U * np.stack([np.abs(blk).sum(1), (blk ** 2).sum(1)], axis=1)
            err = np.abs(got["cstat"][:nb].astype(np.float64) - own)
            assert np.all(err <= lim), f"{tag}: cstat is not the statistics of the stored C at " \
                                       f"{np.argwhere(err > lim)[:4].tolist()}: err {err[err > lim][:4].tolist()}"
        if d.want_head:
            p = c * d.headw.astype(np.float64)
            p = np.concatenate([p, np.zeros((d.M, parts * 32 - d.N))], axis=1).reshape(d.M, parts, 32)
            err = np.abs(got["headout"][:parts].astype(np.float64) - p.sum(2).T)
            lim = 34 * U * np.abs(p).sum(2).T
            assert np.all(err <= lim), f"{tag}: headout is not the head of the stored C at " \
                                       f"{np.argwhere(err > lim)[:4].tolist()}: err {err[err > lim][:4].tolist()}"
    if d.want_colsum:
        region("colsum", got["colsum"], (slice(0, s * d.M),), r.colsum.reshape(-1), r.colsum_bound.reshape(-1))
    if d.want_cstat:
        region("cstat", got["cstat"], (slice(0, nb),), r.cstat, r.cstat_bound)


# ---- the case tables ----------------------------------------------------------------------------------------------------
# Shapes: S1 = (200, 136), ldc 136: an interior 16-byte tile and edge tiles both ways for the 64x64, 128x64 and 64x128
# tiles, one interior 128x128 tile, a last row block of 8 rows, a last head part of 8 columns.  S2 = (100, 70), ldc 73,
# odd lda / ldb / ldmask: no 16-byte path anywhere (the dword-load instantiation).  S3 = (1, 5).
# K = 32, 96, 160 (1, 3, 5 K-tiles: the rem = 1 and 3 tails without and with the steady-state loop), 128 (rem = 2),
# 100 (ragged) and 0.
S1 = dict(M=200, N=136)
S2 = dict(M=100, N=70, ldc=73, lda_pad=1, ldb_pad=3)
S3 = dict(M=1, N=5)


def _table():
    t, seed = {}, [100]

    def add(family, name, mode, shape, K, **kw):
        seed[0] += 1
        kw = {**shape, **kw}
        if kw.get("mask") and "ldc" in shape:
            kw.setdefault("ldmask", 71)
        t.setdefault(family, []).append(make(name, mode, kw.pop("M"), kw.pop("N"), K, seed[0], **kw))

    hd = dict(bias=True, act=ACT_RELU, head=True)
    add("head", "head_s1_k160", NT, S1, 160, **hd)
    add("head", "head_s1_k32_nostore", NT, S1, 32, store_c=0, **hd)
    add("head", "head_s1_k128_nostore", NT, S1, 128, store_c=0, **hd)
    add("head", "head_s2_k100", NT, S2, 100, **hd)
    add("head", "head_s2_k96_nostore", NT, S2, 96, store_c=0, **hd)
    add("head", "head_s3_k128", NT, S3, 128, **hd)
    add("head", "head_s3_k32_nostore", NT, S3, 32, store_c=0, **hd)

    add("colsum", "colsum_s1_k96", TN, S1, 96, colsum=True)
    add("colsum", "colsum_s1_k128", TN, S1, 128, colsum=True)
    add("colsum", "colsum_s2_k100", TN, S2, 100, colsum=True)
    add("colsum", "colsum_s3_k32", TN, S3, 32, colsum=True)
    add("colsum", "colsum_wide_k160", TN, dict(M=70, N=300), 160, colsum=True)      # three 128-wide column tiles

    add("splitk", "splitk2_s1_k160", TN, S1, 160, colsum=True, splitk=2)
    add("splitk", "splitk3_s1_k96", TN, S1, 96, colsum=True, splitk=3)
    add("splitk", "splitk3_s2_k160", TN, S2, 160, colsum=True, splitk=3)
    add("splitk", "splitk7_s2_k100", TN, S2, 100, colsum=True, splitk=7)             # splits 4..6 are empty
    add("splitk", "splitk2_wide_k128", TN, dict(M=70, N=300), 128, colsum=True, splitk=2)
    add("splitk", "splitk2_nt_s1_k128", NT, S1, 128, splitk=2)
    add("splitk", "splitk3_nn_s2_k100", NN, S2, 100, splitk=3)

    for rs in (False, True):
        for kind in ("sep", "alias"):
            add("resid", f"resid_s1_k96_{'rs' if rs else 'one'}_{kind}", NT, S1, 96, resid=kind, rscale=rs)
    add("resid", "resid_s1_k160_bias_relu", NT, S1, 160, resid="alias", rscale=True, bias=True, act=ACT_RELU)
    add("resid", "resid_s2_k160_rs_alias", NT, S2, 160, resid="alias", rscale=True)
    add("resid", "resid_s2_k100_one_sep", NN, S2, 100, resid="sep")
    add("resid", "resid_s3_k32_rs_sep", NT, S3, 32, resid="sep", rscale=True)

    add("cstat", "cstat_s1_k128", NT, S1, 128, cstat=True)
    add("cstat", "cstat_s1_k32_bias_relu", NT, S1, 32, cstat=True, bias=True, act=ACT_RELU)
    add("cstat", "cstat_s2_k100", NT, S2, 100, cstat=True)
    add("cstat", "cstat_s2_k160_bias_relu", NN, S2, 160, cstat=True, bias=True, act=ACT_RELU)
    add("cstat", "cstat_s3_k96_bias_relu", NT, S3, 96, cstat=True, bias=True, act=ACT_RELU)

    add("mask", "mask_s1_k96", NN, S1, 96, mask=True)
    add("mask", "mask_s1_k160_bias_relu", NT, S1, 160, mask=True, bias=True, act=ACT_RELU)
    add("mask", "mask_s2_k100", NN, S2, 100, mask=True)
    add("mask", "mask_s3_k32", NT, S3, 32, mask=True)

    add("apro", "apro_s1_k32", NT, S1, 32, apro=True)
    add("apro", "apro_s1_k96_resid", NT, S1, 96, apro=True, resid="alias", rscale=True)
    add("apro", "apro_s1_k96_bias_cstat", NT, S1, 96, apro=True, bias=True, cstat=True)
    add("apro", "apro_s3_k32", NT, S3, 32, apro=True)

    add("onebuf", "onebuf_s1_k160", NT, S1, 160, bias=True, act=ACT_RELU, cstat=True)
    add("onebuf", "onebuf_s1_k32_tn", TN, S1, 32, colsum=True)
    add("onebuf", "onebuf_s2_k96", NT, S2, 96, bias=True, act=ACT_RELU, cstat=True)   # unaligned: the usual schedule runs

    add("k0", "k0_s1_bias_relu", NT, S1, 0, bias=True, act=ACT_RELU)
    add("k0", "k0_s2_bias", NT, S2, 0, bias=True)
    add("k0", "k0_s3_bias_relu", NT, S3, 0, bias=True, act=ACT_RELU)

    t["gather"] = [make_gathered("gather_n72", 900), make_gathered("gather_n64", 902, N=64)]

    # mask / resid with cstat / head: interior 16-byte tiles and edge tiles of S1 would follow two definitions (refused)
    add("combo", "combo_mask_cstat", NT, S1, 96, mask=True, cstat=True)
    add("combo", "combo_mask_head", NT, S1, 96, mask=True, head=True)
    add("combo", "combo_resid_cstat", NT, S1, 96, resid="sep", rscale=True, cstat=True)
    add("combo", "combo_resid_head", NT, S1, 96, resid="alias", rscale=True, head=True)

    # groups: different modes, epilogues and sizes in one launch (block_start of every problem matters)
    add("group4", "g4_nt_head", NT, S1, 96, **hd)
    add("group4", "g4_nn_mask", NN, S2, 100, mask=True)
    add("group4", "g4_tn_colsum", TN, dict(M=70, N=130), 160, colsum=True)
    add("group4", "g4_nt_m1", NT, dict(M=1, N=40), 32, bias=True)
    add("group4v", "g4v_nt_head", NT, S1, 96, **hd)                                   # all 16-byte readable
    add("group4v", "g4v_nn_mask", NN, dict(M=132, N=72), 128, mask=True)
    add("group4v", "g4v_tn_colsum", TN, dict(M=72, N=132), 160, colsum=True)
    add("group4v", "g4v_nt_m1", NT, dict(M=1, N=40), 32, bias=True)
    add("group8", "g8_nt_head_nostore", NT, S1, 32, store_c=0, **hd)
    add("group8", "g8_nn_mask", NN, dict(M=132, N=72), 96, mask=True)
    add("group8", "g8_tn_colsum_split3", TN, dict(M=72, N=132), 160, colsum=True, splitk=3)
    add("group8", "g8_nt_m1", NT, dict(M=1, N=40), 128, bias=True)
    add("group8", "g8_nt_resid", NT, dict(M=68, N=64), 64, resid="alias", rscale=True)
    add("group8", "g8_nt_cstat", NT, dict(M=100, N=72), 96, cstat=True, bias=True, act=ACT_RELU)
    add("group8", "g8_nt_k0", NT, dict(M=40, N=36), 0, bias=True)
    add("group8", "g8_tn_plain", TN, dict(M=64, N=64), 32)

    rd = dict(exact=False)
    add("rounded", "r_head", NT, S1, 160, bias=True, act=ACT_TANH, head=True, **rd)
    add("rounded", "r_colsum", TN, S1, 160, colsum=True, **rd)
    add("rounded", "r_splitk3", TN, S1, 160, colsum=True, splitk=3, **rd)
    add("rounded", "r_resid", NT, S1, 160, bias=True, act=ACT_TANH, resid="alias", rscale=True, **rd)
    add("rounded", "r_cstat", NT, S1, 160, bias=True, act=ACT_TANH, cstat=True, **rd)
    add("rounded", "r_mask", NN, S1, 160, bias=True, act=ACT_TANH, mask=True, **rd)
    add("rounded_apro", "r_apro", NT, S1, 160, apro=True, bias=True, act=ACT_TANH, resid="alias", rscale=True, **rd)
    t["rounded"].append(make_gathered("r_gather", 904, exact=False))
    return t


TABLE = _table()
CASES = {d.name: d for fam in TABLE.values() for d in fam}
assert len(CASES) == sum(len(f) for f in TABLE.values())


def names(*families):
    return [d.name for f in families for d in TABLE[f]]


@lru_cache(maxsize=None)
def ref(name):
    """The reference of a case, computed once and shared by every tile / schedule that runs it (treat as read-only)."""
    return reference(CASES[name])
