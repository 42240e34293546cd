"""The acceptance rule of the fp32 encoder test (tests/test_encoder_fp32_gpu.py), checked on the CPU.  No kernel runs here
and no faulty kernel is built: the faults are switches of the oracle (oracle/fasternet_oracle.py, `mutate=`).

The rule: `oracle/bf16_accept.accept(kind="rel", cap=CAP_REL_FP32)` per element of both stage outputs (every position and
channel), of the pooled vector, the pre-head features, the features and the running statistics.  `got` may be 4 x d_ref
from forward_faithful(mode=None, accum=np.float64) on the maximum and on the mean of |got - ref| / rms(ref), d_ref being the
distance of the accum=np.float32 run from it, floor 2e-6, and under a cap of 2.5e-4 on the maximum whatever d_ref says.
With mode=None and fp64 products the faithful oracle is `forward` (tests/test_bf16_oracle.py ties the two to 1e-12).

What the suite had for this path compares pooled FEATURES, max|got - ref| / max|ref| < 2e-5: a mean over P2 positions
(1440 per sample at 360 x 256) behind two dense layers.  Measured here (weights seed 11, inputs seed 21, train mode,
"stages.2" = max of |got - ref| / rms over all positions and channels):
    360 x 256 b7   d_ref stages.2 1.15e-5                      -> bound 4.6e-5
    last_position  features 9.3e-6 (passes 2e-5)   stages.2 6.8e-3   148 x the bound
    corner_tap     features 5.4e-6 (passes 2e-5)   stages.2 4.0e-3    87 x the bound
    84 x 84 b5     d_ref stages.2 6.6e-6                       -> bound 2.7e-5
    halo_zero 0.21, droppath_row 0.85, ragged_tile 4.1, tap_transposed 0.48, merge_rows 17.8: 8e3 x the bound and more
    (their features move by 9e-3 to 0.8: the pooled check saw these already)
At 360 x 256 b2 the DropPath pattern keeps the faulty block's residual of the last sample and corner_tap reaches the
features there (1.7e-4, 0.10 per position); at b7 that residual is dropped and only the second block's conv shows them: whether the pooled check
notices depends on such accidents.
A partial conv that never writes the last position of the last sample, or drops one tap there, passes the pooled check at
the reference's own geometry; per position both sit two decades beyond what a correct implementation is allowed.
"""
import numpy as np
import pytest

from helpers import encoder_fp32_cases as EC
from helpers.encoder_fp32_cases import BA, FO

ALL_TAPS = EC.STAGE_TAPS + EC.FP32_TAPS


def old_rule(got, ref):
    """What the suite had: features within 2e-5 of the largest feature magnitude."""
    return float(np.abs(got["features"] - ref["features"]).max() / np.abs(ref["features"]).max())


@pytest.mark.parametrize("name", [c.name for c in EC.CASES])
def test_the_oracle_pair_differs_and_stays_a_quarter_under_the_cap(name):
    """fp32 products are another realisation, not the same numbers (d_ref > 0), and at every shape of the GPU test
    4 x d_ref stays under the cap, so no comparison there is vacuous."""
    orc, secs = EC.oracle_pair(name)
    print(f"\n== {name}: oracle pair, train + eval, {secs:.1f} s")
    for phase in ("train", "eval"):
        for k in ALL_TAPS:
            d = BA.rel_stats(orc["fp32"][phase][k], orc["fp64"][phase][k])
            print(f"{phase} {k:18s} d_ref {d['max']:.3g} / {d['mean']:.3g}")
            assert 0.0 < d["max"] <= EC.CAP / 4, (phase, k, d)
    s, s32 = orc["fp64"]["stats"], orc["fp32"]["stats"]
    for k in s:
        if k.endswith("running_var"):
            km = k.replace("running_var", "running_mean")
            assert BA.rel_stats(s32[k], s[k])["max"] <= EC.CAP / 4, k
            assert BA.rel_stats(s32[km], s[km], float(np.sqrt(s[k].max())))["max"] <= EC.CAP / 4, km


@pytest.mark.parametrize("name", EC.SMALL)
@pytest.mark.parametrize("perm_seed", [1, 2])
def test_accept_passes_a_second_correct_fp32_implementation(name, perm_seed):
    orc, _ = EC.oracle_pair(name)
    got = {}
    got["train"], got["stats"] = EC.oracle(name, True, accum=np.float32, perm_seed=perm_seed)
    got["eval"], _ = EC.oracle(name, False, accum=np.float32, perm_seed=perm_seed, stats=got["stats"])
    bad = EC.compare(got, orc)
    assert not bad, bad
    # and the yardstick run itself sits exactly at d_ref
    ok, rep = BA.accept(orc["fp32"]["train"]["stages.2"], orc["fp64"]["train"]["stages.2"], orc["fp32"]["train"]["stages.2"],
                        kind="rel", cap=EC.CAP)
    assert ok and rep["got"] == rep["d_ref"]


def test_the_cap_is_off_by_default_and_holds_whatever_d_ref_says():
    ref = EC.oracle_train("40x64-b3", "fp64")[0]["stages.2"]
    rms = np.sqrt(np.mean(ref ** 2))
    wave = np.sign(np.sin(np.arange(ref.size).reshape(ref.shape)))
    noisy = ref + 1e-4 * rms * wave                   # a yardstick of 1e-4: 4 x d_ref is beyond the cap
    off = ref + 3e-4 * rms * wave                     # within 4 x that yardstick, beyond the cap
    ok, rep = BA.accept(off, ref, noisy, kind="rel")
    assert ok, rep                                    # without a cap the rule follows d_ref, as the bf16 tests use it
    ok, rep = BA.accept(off, ref, noisy, kind="rel", cap=EC.CAP)
    assert not ok and any("VACUOUS" in w for w in rep["why"]) and any(w.startswith("cap:") for w in rep["why"]), rep
    ok, rep = BA.accept(ref, ref, noisy, kind="rel", cap=EC.CAP)
    assert not ok and any("VACUOUS" in w for w in rep["why"]), rep      # vacuous even when got is exact


def _stage2(name, mutant):
    """-> (old pooled-feature figure, report of the new rule on the stages.2 tap) of a mutant in train mode."""
    ref, ref32 = EC.oracle_train(name, "fp64")[0], EC.oracle_train(name, "fp32")[0]
    bad, _ = EC.oracle(name, True, mutate=(mutant,))
    assert np.array_equal(bad["stages.0"], ref["stages.0"])           # the faults sit behind stage 1
    ok, rep = BA.accept(bad["stages.2"], ref["stages.2"], ref32["stages.2"], kind="rel", cap=EC.CAP)
    old = old_rule(bad, ref)
    print(BA.fmt(mutant, rep), f" features={old:.3g}  max / bound = {rep['got']['max'] / rep['bound']['max']:.3g}")
    return old, ok, rep


@pytest.mark.parametrize("mutant", FO.LOCAL_MUTANTS)
def test_a_fault_at_one_position_passes_the_pooled_check_and_fails_per_position(mutant):
    old, ok, rep = _stage2("360x256-b7", mutant)
    assert old < 2e-5, old                    # the pooled check the suite had does not notice
    assert not ok, rep
    assert rep["got"]["max"] / rep["bound"]["max"] > 10, rep
    # one position of 1440 per sample (and what the next block's 3x3 window spreads it to): the mean stays inside its bound, only
    # a per-element maximum sees the fault
    assert rep["got"]["mean"] <= rep["bound"]["mean"], rep


@pytest.mark.parametrize("mutant", FO.MUTANTS)
def test_the_gross_faults_are_rejected_per_position_too(mutant):
    old, ok, rep = _stage2("84x84-b5", mutant)
    assert not ok, rep
    assert rep["got"]["max"] / rep["bound"]["max"] > 10, rep
