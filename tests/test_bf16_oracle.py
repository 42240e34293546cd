"""The bf16-faithful oracle (oracle/fasternet_oracle.py:forward_faithful) and the acceptance rule of the bf16 encoder
tests (oracle/bf16_accept.py), checked on the CPU:
  * the numpy bf16 rounding helper is torch's `.bfloat16()`, bit for bit, edge cases included;
  * with every rounding off the NHWC restatement equals the NCHW `forward` that tests/test_oracle_golden.py pins to the
    reference, taps and features, to 1e-12;
  * `accept` passes a correct implementation (the fp32-product variant with another summation order) and REJECTS five
    deliberate faults switched on inside the oracle's stage-2 path, each of a kind a kernel could have.  No faulty kernel
    is built: the faults are switches of the oracle (`mutate=`).

Measured with FasterNet's own initialiser (seed 14, inputs 24: the 84 x 84, batch 5 case of the GPU test), train mode,
on the "stages.2" tap: max steps / share beyond one step / mean steps, and `feat` = the metric the suite had before,
largest feature difference over the largest feature, which has to exceed 3e-2 to be noticed at all:
    two correct realisations (d_ref)   2.82 / 0.45 % / 0.023        -> bound 11.3 / 1.8 % / 0.092
    halo_zero                          58.3 / 21.5 % / 1.5          feat 0.012   (missed by the old bound)
    droppath_row                       377  / 5.0 %  / 1.12         feat 0.040
    ragged_tile                        758  / 55.7 % / 12.7         feat 0.74    (a whole sample of five loses its blocks)
    tap_transposed                     107  / 59.4 % / 4.31         feat 0.022   (missed by the old bound)
    merge_rows                         2570 / 98.8 % / 178          feat 0.67
Every fault is beyond its bound by more than a factor of ten on at least one statistic.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "oracle"))
import bf16_accept as BA          # noqa: E402
import fasternet_oracle as FO     # noqa: E402

TAPS16 = ("stages.0", "stages.2")


def module_weights(seed, angle_bins, dist_bins, mode="bf16", max_batch=8):
    from porl_amd.agent.fasternet import FasterNet
    torch.manual_seed(seed)
    m = FasterNet(3, 256, max_batch=max_batch, angle_bins=angle_bins, dist_bins=dist_bins, compute_dtype=mode)
    return {k: v.cpu().numpy().copy() for k, v in m.state_dict().items()}


def run(sd, st, scale, training=True, **kw):
    stats = {k: v.copy() for k, v in sd.items() if "running" in k}
    taps = {}
    feat = FO.forward_faithful(sd, stats, st.copy(), training, scale if training else None, taps=taps, **kw)
    taps["features"] = feat
    return taps, stats


def test_rounding_helper_is_torch_bfloat16():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(100000) * np.exp(rng.uniform(-30, 30, 100000))).astype(np.float32)
    u = lambda bits: np.array(bits, dtype=np.uint32).view(np.float32)
    edge = np.concatenate([
        u([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000]),       # exact ties: down to even, up to even, both signs
        u([0x3F808001, 0x3F807FFF]),                               # just past / just short of a tie
        u([0x00000000, 0x80000000]),                               # +-0
        u([0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00800000]),   # subnormals and the first normal
        u([0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000]),               # largest finite values
        u([0x7F800000, 0xFF800000]),                               # inf
    ])
    for v in (x, edge):
        want = torch.from_numpy(v).bfloat16().float().numpy()
        got = FO.bf16_round(v).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(FO.bf16_round(np.array([np.nan], dtype=np.float32))).all()
    t = FO.bf16_round(u([0x3F808000, 0x3F818000]))
    assert t[0] == 1.0 and t[1] == 1.0 + 2.0 ** -6                 # the ties really went to even
    assert np.isinf(FO.bf16_round(u([0x7F7F8000]))[0])             # and the top of the range rounds to inf like torch


@pytest.mark.parametrize("ab,db,B", [(40, 64, 3), (84, 84, 5), (360, 256, 2)])
def test_without_rounding_it_is_the_pinned_fp64_oracle(ab, db, B):
    sd = module_weights(7, ab, db)
    st, scale = BA.make_inputs(ab, B, 3)
    nhwc = lambda t: t.transpose(0, 2, 3, 1).reshape(-1, t.shape[1])
    for training in (True, False):
        s_ref = {k: v.copy() for k, v in sd.items() if "running" in k}
        t_ref = {}
        x_ref = st.copy()
        f_ref = FO.forward(sd, s_ref, x_ref, training, scale if training else None, taps=t_ref, angle_bins=ab, dist_bins=db)
        got, s_got = run(sd, st, scale, training, mode=None, angle_bins=ab, dist_bins=db)
        rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
        assert rel(got["features"], f_ref) < 1e-12
        for k in ("patch_embed", "stages.0", "stages.1", "stages.2"):
            assert rel(got[k], nhwc(t_ref[k])) < 1e-12, k
        assert rel(got["avgpool_pre_head"], t_ref["avgpool_pre_head"]) < 1e-12
        for k in s_ref:
            if k.endswith("num_batches_tracked"):
                assert int(s_got[k]) == int(s_ref[k])
            else:
                assert np.abs(s_got[k].astype(np.float64) - s_ref[k]).max() <= 1e-6 * np.abs(s_ref[k]).max(), k
        if not training:
            assert x_ref[B // 2, 7] == 0.0


@pytest.fixture(scope="module")
def case84():
    ab = db = 84
    sd = module_weights(14, ab, db)
    st, scale = BA.make_inputs(ab, 5, 24)               # the 84 x 84 case of tests/test_encoder_bf16_gpu.py
    ref, _ = run(sd, st, scale, mode="bf16", angle_bins=ab, dist_bins=db)
    ref32, _ = run(sd, st, scale, mode="bf16", accum=np.float32, angle_bins=ab, dist_bins=db)
    return sd, st, scale, ref, ref32


def old_rule(got, ref):
    """What the suite had: pooled features within 3e-2 of the largest feature magnitude."""
    return float(np.abs(got["features"] - ref["features"]).max() / np.abs(ref["features"]).max())


def test_accept_passes_a_second_correct_implementation(case84):
    sd, st, scale, ref, ref32 = case84
    for seed in (1, 2):
        other, _ = run(sd, st, scale, mode="bf16", accum=np.float32, perm_seed=seed, angle_bins=84, dist_bins=84)
        for k in TAPS16:
            ok, rep = BA.accept(other[k], ref[k], ref32[k])
            print(BA.fmt(f"perm{seed} {k}", rep))
            assert ok, (k, rep)
            # the oracle pair alone stays at or below a quarter of the caps, so the GPU test at this shape is not vacuous
            assert rep["d_ref"]["max"] <= BA.CAP_MAX_STEPS / 4 and rep["d_ref"]["share"] <= BA.CAP_SHARE / 4, (k, rep)
        for k in ("pooled", "avgpool_pre_head", "features"):
            ok, rep = BA.accept(other[k], ref[k], ref32[k], kind="rel")
            print(BA.fmt(f"perm{seed} {k}", rep))
            assert ok, (k, rep)
    ok, rep = BA.accept(ref32["stages.2"], ref["stages.2"], ref32["stages.2"])
    assert ok and rep["got"] == rep["d_ref"]


def test_accept_fails_as_vacuous_when_the_yardstick_is_too_long(case84):
    _, _, _, ref, _ = case84
    r = ref["stages.2"]
    noisy = r * (1 + 2.0 ** -8 * 5 * np.sign(np.sin(np.arange(r.size).reshape(r.shape))))      # ~5 steps everywhere
    ok, rep = BA.accept(r, r, noisy)
    assert not ok and any("VACUOUS" in w for w in rep["why"])


@pytest.mark.parametrize("mutant", FO.MUTANTS)
def test_accept_rejects_a_faulty_stage2(case84, mutant):
    sd, st, scale, ref, ref32 = case84
    bad, _ = run(sd, st, scale, mode="bf16", mutate=(mutant,), angle_bins=84, dist_bins=84)
    assert np.array_equal(bad["stages.0"], ref["stages.0"])           # the faults sit behind stage 1
    s = BA.steps(bad["stages.2"], ref["stages.2"])
    moved = float(np.mean(s > 1.0))
    ok, rep = BA.accept(bad["stages.2"], ref["stages.2"], ref32["stages.2"])
    print(BA.fmt(mutant, rep), f" feat={old_rule(bad, ref):.3g}")
    if mutant == "tap_transposed":
        # the weakest of the five: make sure it is a fault worth the name before asking for its rejection
        assert moved >= 0.03, moved
    assert not ok, rep
    # and the margin: the fault's signature is more than a decade beyond what a correct implementation is allowed
    assert max(rep["got"][k] / rep["bound"][k] for k in rep["bound"]) > 10, rep
    if mutant in ("halo_zero", "tap_transposed"):
        assert old_rule(bad, ref) < 3e-2          # what the suite had before does not notice these two
