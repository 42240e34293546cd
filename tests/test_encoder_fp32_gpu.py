"""The encoder's fp32 kernels (csrc/encoder.hpp, the encoder's use of csrc/gemm_f32.hpp, the dispatch in
csrc/encoder_api.inc) per POSITION against the fp64 oracle — oracle/fasternet_oracle.py:forward_faithful(mode=None) —
instead of per pooled feature (2e-5 in tests/test_fasternet_gpu.py and tests/test_config5_gpu.py, which stay).  What is
compared, after one train-mode forward with explicit DropPath factors that differ between neighbouring samples
(kept-and-rescaled, dropped, untouched) and one eval-mode forward behind it: the stage-1 and stage-2 outputs
(FasterNet.taps(): every row and channel), the pooled vector, the pre-head features, the features, after the train forward
every running statistic and num_batches_tracked, and the in-place clamp of the one state entry above 8.

Rule (oracle/bf16_accept.py, kind="rel" with cap=CAP_REL_FP32; tests/test_fp32_oracle.py shows on the CPU that it rejects
a partial conv that leaves one position unwritten or drops one tap there — both pass the pooled 2e-5 check at 360 x 256
b7 — and the five gross faults of tests/test_bf16_oracle.py): per element |got - ref| / rms(ref) may be 4 x d_ref on the
maximum and on the mean, d_ref being the distance of the oracle's fp32-product run from its fp64-product run, floor 2e-6;
a maximum beyond 2.5e-4 fails whatever d_ref says and 4 x d_ref beyond 2.5e-4 fails as vacuous.  running_mean is measured
on the scale sqrt(max running_var) of its layer.

Cases (tests/helpers/encoder_fp32_cases.py; weights seed 11, inputs seed 21) and the branch each one reaches, asserted
through the launch record (engine.prof_enable / prof_read) by name AND count, the replaced kernel being absent:
  40x64 b3      10 x 16 grid, rows1 = 480 (ragged 128- and 64-row GEMM tiles); partial conv = im2col3x3_kernel + GEMM; merge
                through the grouped-row gather (no space_to_depth_kernel)
  84x84 b5      21 x 21 grid: the odd grid forces space_to_depth_kernel and the 21 -> 10 floor; rows2 = 500
  360x256 b2    reference geometry: pconv3x3_kernel<24,24,64> (90 rows in 4-row tiles, last tile 2 rows) and <48,48,32>
                (45 rows in 8-row tiles, last tile 5 rows), sparse patch embedding (patch_bn_kernel), merge gather
  360x256 b7    odd batch; last sample and last position
  40x64 embed 64, depths (2, 1), n_div 4, mlp_ratio 2, b2       general block loop, cp = 16
  40x64 embed 32, depths (1, 1), n_div 2, mlp_ratio 3.0, b2     cp = 16 / 32 with n_div 2, two blocks.  Its hidden widths are
                96 / 192, both multiples of the 32-wide K tile, so enc_block's fold condition is TRUE here (asserted: four
                products with the operand prologue, bn_apply_kernel for the merge alone); the unfolded branch is the next case
  40x64 embed 32, depths (1, 1), n_div 2, mlp_ratio 2.25, b2    hidden 72 / 144, no multiples of 32: the fold condition is
                false, BatchNorm runs as a separate bn_apply_kernel sweep per block, no product has the operand prologue
Variants (engine.tune_set before the module is built, restored in `finally`): enc_pconv_mfma=1 (pconv_f32_mfma_kernel,
neither pconv3x3_kernel nor im2col3x3_kernel), enc_dense_patch=1 (patch_embed_kernel + colstats_partial_kernel +
bn_apply_kernel, no patch_bn_kernel), enc_s2d=1 (space_to_depth_kernel where the gather ran), enc_bn_sweep=1 (bn_apply_kernel
per block, no product with the operand prologue), enc_patch_rows=16 (row blocks 16 + 5 at 84 x 84, 5 x 16 + 10 at 360 x 256).
patch_bn_kernel's grid is not in the launch record and the row count changes no other observable: for enc_patch_rows the
record only shows that patch_bn_kernel ran; what the case adds is that every position behind the ragged last row block is
compared.

Measured on MI355X, max / mean of |. - ref| / rms(ref): d_ref = the oracle's fp32-product run, kernels = what is under test;
the last column is the largest running_var / running_mean figure after the train forward (their d_ref is 0 or one fp32
ulp, 6.6e-8, so the 2e-6 floor is their bound).  The kernels sit AT d_ref everywhere — the largest ratio to d_ref is 2.4
(84x84 train features), against the 4 allowed — so the oracle needed no fp32 coefficients or 32-row statistics beyond what
accum=np.float32 already does, and no per-position excess showed at any case: no kernel was changed.  The oracle pair of
360x256 b7, train + eval, took 0.6 s there.
                                        stages.0         stages.2         pooled           pre_head         features         running stats
40x64-b3 d_ref train                    2.2e-6/2.7e-8    5.3e-6/2.3e-7    9.7e-7/2.4e-7    2.6e-6/2.2e-7    2.5e-6/4.7e-7
40x64-b3 d_ref eval                     3.2e-6/2.1e-8    5.0e-6/2.8e-7    1.5e-6/3.5e-7    2.9e-6/2.9e-7    2.3e-6/5.2e-7
40x64-b3 kernels train                  1.6e-6/2.8e-8    5.8e-6/2.2e-7    1.0e-6/2.3e-7    2.7e-6/2.1e-7    3.0e-6/4.6e-7    6.6e-8 / 4.8e-9
40x64-b3 kernels eval                   2.6e-6/2.0e-8    7.0e-6/2.8e-7    1.5e-6/3.6e-7    2.8e-6/2.9e-7    2.4e-6/5.3e-7
84x84-b5 d_ref train                    2.6e-6/2.4e-8    6.7e-6/2.1e-7    1.0e-6/2.0e-7    2.5e-6/2.0e-7    1.5e-6/3.3e-7
84x84-b5 d_ref eval                     2.2e-6/2.0e-8    5.9e-6/2.8e-7    2.4e-6/4.3e-7    3.0e-6/3.4e-7    1.9e-6/4.7e-7
84x84-b5 kernels train                  2.7e-6/2.4e-8    5.8e-6/2.1e-7    1.0e-6/2.0e-7    3.2e-6/2.0e-7    3.7e-6/4.4e-7    6.6e-8 / 4.8e-9
84x84-b5 kernels eval                   2.2e-6/1.8e-8    6.7e-6/2.8e-7    2.4e-6/4.1e-7    3.1e-6/3.3e-7    2.5e-6/5.2e-7
360x256-b2 d_ref train                  4.4e-6/1.6e-8    1.4e-5/1.5e-7    8.7e-7/2.2e-7    2.6e-6/2.1e-7    1.7e-6/4.2e-7
360x256-b2 d_ref eval                   6.6e-6/1.7e-8    1.2e-5/3.8e-7    3.1e-6/8.1e-7    5.1e-6/6.0e-7    4.2e-6/8.7e-7
360x256-b2 kernels train                4.4e-6/1.6e-8    1.2e-5/1.5e-7    8.0e-7/2.1e-7    2.1e-6/2.0e-7    1.8e-6/4.3e-7    6.6e-8 / 2.4e-9
360x256-b2 kernels eval                 6.6e-6/1.5e-8    1.2e-5/3.5e-7    2.7e-6/7.2e-7    4.7e-6/5.4e-7    3.4e-6/8.0e-7
360x256-b7 d_ref train                  8.3e-6/1.9e-8    1.2e-5/1.5e-7    9.0e-7/1.6e-7    3.1e-6/1.8e-7    1.7e-6/3.1e-7
360x256-b7 d_ref eval                   5.5e-6/1.6e-8    1.3e-5/2.5e-7    1.7e-6/4.1e-7    3.4e-6/3.1e-7    2.2e-6/4.6e-7
360x256-b7 kernels train                5.8e-6/1.9e-8    1.6e-5/1.5e-7    9.9e-7/1.6e-7    2.8e-6/1.8e-7    3.9e-6/4.0e-7    6.6e-8 / 1.6e-9
360x256-b7 kernels eval                 7.8e-6/1.5e-8    1.2e-5/2.5e-7    1.6e-6/4.1e-7    3.0e-6/3.2e-7    3.5e-6/5.4e-7
40x64-e64-d21-b2 d_ref train            1.6e-6/2.8e-8    3.4e-6/1.7e-7    6.7e-7/2.0e-7    2.6e-6/1.8e-7    3.8e-6/4.3e-7
40x64-e64-d21-b2 d_ref eval             2.3e-6/2.2e-8    4.2e-6/2.4e-7    1.2e-6/3.0e-7    2.0e-6/2.3e-7    2.6e-6/4.6e-7
40x64-e64-d21-b2 kernels train          1.4e-6/2.8e-8    3.6e-6/1.7e-7    7.8e-7/1.9e-7    1.8e-6/1.8e-7    4.5e-6/4.5e-7    6.6e-8 / 2.9e-9
40x64-e64-d21-b2 kernels eval           1.5e-6/2.1e-8    3.5e-6/2.3e-7    1.2e-6/3.0e-7    2.1e-6/2.3e-7    2.1e-6/4.7e-7
40x64-e32-d11-r3-b2 d_ref train         1.2e-6/2.2e-8    1.8e-6/1.3e-7    6.4e-7/1.8e-7    1.7e-6/1.5e-7    3.1e-6/3.6e-7
40x64-e32-d11-r3-b2 d_ref eval          1.4e-6/1.8e-8    2.2e-6/2.1e-7    1.2e-6/3.1e-7    1.9e-6/2.4e-7    2.2e-6/4.7e-7
40x64-e32-d11-r3-b2 kernels train       1.2e-6/2.0e-8    1.7e-6/1.3e-7    6.3e-7/1.8e-7    2.1e-6/1.5e-7    3.9e-6/3.7e-7    6.6e-8 / 2.0e-9
40x64-e32-d11-r3-b2 kernels eval        1.8e-6/1.8e-8    2.3e-6/2.0e-7    1.0e-6/2.8e-7    1.8e-6/2.1e-7    2.6e-6/4.5e-7
40x64-e32-d11-r2.25-b2 d_ref train      1.2e-6/2.0e-8    1.8e-6/1.3e-7    7.7e-7/2.0e-7    1.5e-6/1.7e-7    2.4e-6/4.1e-7
40x64-e32-d11-r2.25-b2 d_ref eval       2.3e-6/1.8e-8    2.0e-6/2.2e-7    9.2e-7/3.3e-7    2.0e-6/2.4e-7    2.4e-6/4.9e-7
40x64-e32-d11-r2.25-b2 kernels train    9.9e-7/1.9e-8    1.6e-6/1.2e-7    6.2e-7/1.9e-7    1.7e-6/1.6e-7    2.5e-6/3.9e-7    6.6e-8 / 1.5e-9
40x64-e32-d11-r2.25-b2 kernels eval     2.3e-6/1.7e-8    2.0e-6/1.8e-7    7.9e-7/2.5e-7    1.6e-6/2.0e-7    2.8e-6/4.3e-7
variants, kernels (d_ref is that of the case):
  enc_pconv_mfma=1 360x256-b2 train     4.4e-6/1.6e-8    1.2e-5/1.5e-7    8.0e-7/2.0e-7    2.1e-6/2.0e-7    2.3e-6/4.3e-7    6.6e-8 / 2.5e-9
  enc_pconv_mfma=1 360x256-b2 eval      6.6e-6/1.5e-8    1.2e-5/3.5e-7    2.8e-6/7.2e-7    4.7e-6/5.4e-7    3.5e-6/7.9e-7
  enc_pconv_mfma=1 84x84-b5 train       2.7e-6/2.4e-8    5.8e-6/2.1e-7    1.0e-6/2.0e-7    3.2e-6/2.0e-7    3.7e-6/4.4e-7    6.6e-8 / 4.8e-9
  enc_pconv_mfma=1 84x84-b5 eval        2.2e-6/1.8e-8    6.7e-6/2.8e-7    2.4e-6/4.1e-7    3.1e-6/3.3e-7    2.5e-6/5.2e-7
    (at 84x84 the default is the patch-matrix GEMM, which walks k = (ky, kx, ci) on the same matrix pipe: same figures)
  enc_dense_patch=1, enc_s2d=1, enc_bn_sweep=1, enc_patch_rows=16 at 360x256-b2: every figure equals the 360x256-b2
    "kernels" rows above, and enc_dense_patch=1, enc_patch_rows=16 at 84x84-b5 the 84x84-b5 rows, to the three digits
    printed (tests/test_fasternet_gpu.py holds these variants to the default bit for bit or to 1e-6 of the features)
"""
import re

import numpy as np
import pytest
import torch

from helpers import encoder_fp32_cases as EC

pytestmark = pytest.mark.gpu

TUNE_DEFAULTS = {"enc_pconv_mfma": 0, "enc_dense_patch": 0, "enc_s2d": 0, "enc_bn_sweep": 0, "enc_patch_rows": 0}

# launches of one train + one eval forward, by profile label.  "apro" = grouped fp32 GEMM launches whose label carries the
# operand prologue (BatchNorm + ReLU folded into W2's staging).  bn_apply_kernel: once per forward for the merge's
# BatchNorm, once more per block that does not fold, and once more for the dense patch embedding's BatchNorm.
BASE = dict(patch_bn_kernel=2, patch_stats_kernel=1, patch_embed_kernel=0, colstats_partial_kernel=0, pconv3x3_kernel=0,
            im2col3x3_kernel=0, pconv_f32_mfma_kernel=0, space_to_depth_kernel=0, bn_apply_kernel=2, apro=6, gap_kernel=2)
LAUNCHES = {
    "40x64-b3": dict(im2col3x3_kernel=6),
    "84x84-b5": dict(im2col3x3_kernel=6, space_to_depth_kernel=2),
    "360x256-b2": dict(pconv3x3_kernel=6),
    "360x256-b7": dict(pconv3x3_kernel=6),
    "40x64-e64-d21-b2": dict(im2col3x3_kernel=6),
    "40x64-e32-d11-r3-b2": dict(im2col3x3_kernel=4, apro=4),
    "40x64-e32-d11-r2.25-b2": dict(im2col3x3_kernel=4, bn_apply_kernel=2 + 4, apro=0),
}
VARIANT_LAUNCHES = {
    "enc_pconv_mfma": dict(pconv_f32_mfma_kernel=6, pconv3x3_kernel=0, im2col3x3_kernel=0),
    "enc_dense_patch": dict(patch_embed_kernel=2, colstats_partial_kernel=1, patch_bn_kernel=0, patch_stats_kernel=0,
                            bn_apply_kernel=2 + 2),
    "enc_s2d": dict(space_to_depth_kernel=2),
    "enc_bn_sweep": dict(bn_apply_kernel=2 + 6, apro=0),
    "enc_patch_rows": dict(),
}
VARIANTS = [
    ("360x256-b2", "enc_pconv_mfma", 1), ("84x84-b5", "enc_pconv_mfma", 1),
    ("360x256-b2", "enc_dense_patch", 1), ("84x84-b5", "enc_dense_patch", 1),
    ("360x256-b2", "enc_s2d", 1),
    ("360x256-b2", "enc_bn_sweep", 1),
    ("84x84-b5", "enc_patch_rows", 16), ("360x256-b2", "enc_patch_rows", 16),
]
GEMM = re.compile(r"gemm_f32_kernel<\d+,\d+,\d+,\d+,\d+,(true|false),(true|false)")


def launch_counts(prof):
    counts = {k: 0 for k in BASE}
    for p in prof:
        if not p["launches"]:
            continue
        assert "bf16" not in p["name"], p["name"]                     # the fp32 mode runs no bf16 kernel
        g = GEMM.search(p["name"])
        if g:
            counts["apro"] += p["launches"] if g.group(2) == "true" else 0
            continue
        for k in BASE:
            if p["name"].endswith(k):
                counts[k] += p["launches"]
    return counts


def run_case(name, tune=None):
    from porl_amd import engine as E
    case = EC.BY_NAME[name]
    dev = torch.device("cuda")
    want = dict(BASE, **LAUNCHES[name])
    try:
        if tune:
            E.tune_set(*tune)                                         # engines copy the process defaults when created
            want.update(VARIANT_LAUNCHES[tune[0]])
        m = EC.make_module(case, dev)
    finally:
        if tune:
            E.tune_set(tune[0], TUNE_DEFAULTS[tune[0]])
    st, scale = EC.inputs(name)
    assert len(set(scale[:, 0])) > 1 and (scale[:, :-1] != scale[:, 1:]).all() and (scale == 0).any(axis=1).all()
    assert (st > 8).sum() == 1 and st[case.B // 2, 7] > 8

    # preconditions: fp32 taps of the expected shape
    Hp, Wp = case.ab // 4, case.db // 4
    shapes = {"stages.0": (Hp * Wp, case.embed), "stages.2": ((Hp // 2) * (Wp // 2), 2 * case.embed),
              "pooled": (1, 2 * case.embed), "avgpool_pre_head": (1, 1280)}
    for tap in m.TAP_NAMES:
        _, rps, cols, eb = m.tap_info(tap)
        assert eb == 4 and (rps, cols) == shapes[tap], (tap, rps, cols, eb)

    got = {}
    E.prof_enable(True)
    try:
        for phase in ("train", "eval"):
            m.train(phase == "train")
            x = torch.from_numpy(st.copy()).to(dev)
            feat = m(x, drop_scale=torch.from_numpy(scale)) if phase == "train" else m(x)
            torch.cuda.synchronize()
            taps = {k: v.cpu().numpy().astype(np.float64) for k, v in m.taps(case.B).items()}
            assert all(v.dtype == torch.float32 for v in m.taps(case.B).values())
            taps["features"] = feat.cpu().numpy().astype(np.float64)
            got[phase] = taps
            clamped = st.copy()
            clamped[case.B // 2, 7] = 0.0
            assert np.array_equal(x.cpu().numpy(), clamped)          # the in-place clamp of the entry > 8, nothing else
            if phase == "train":
                got["stats"] = {k: v.cpu().numpy().copy() for k, v in m.state_dict().items() if "running" in k or "tracked" in k}
        prof = E.prof_read(512)
    finally:
        E.prof_enable(False)

    # the branch this case means to test is the one that ran
    counts = launch_counts(prof)
    assert counts == want, {k: (counts[k], want[k]) for k in want if counts[k] != want[k]}

    orc, secs = EC.oracle_pair(name)
    print(f"\n== fp32 {name} {tune or ''}: oracle (fp64 + fp32 products, train + eval) {secs:.1f} s")
    bad = EC.compare(got, orc)
    assert not bad, bad


@pytest.mark.parametrize("name", [c.name for c in EC.CASES])
def test_kernels_match_the_fp64_oracle_per_position(name):
    run_case(name)


@pytest.mark.parametrize("name,key,value", VARIANTS, ids=[f"{n}-{k}={v}" for n, k, v in VARIANTS])
def test_variant_kernels_match_the_fp64_oracle_per_position(name, key, value):
    run_case(name, (key, value))
