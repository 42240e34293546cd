"""CPU-side checks of the keyed row sampler's host mirror (tests/helpers/sampler_cases.py, the restatement that
tests/test_sampler_gpu.py holds the device to): the scalar and the vectorised form agree, the hash and the domain sit on
fixed points worked out from the constants of csrc/kernels.hpp, the draw is a bijection of [0, n) of which a window is a
slice, and over 200 000 consecutive steps the rows drawn from a small store, and from the two stores that bracket the
smallest domain of the four-round form, are uniform: alone, per batch, in pairs within
a batch, from one step to the next, and in the xor of two positions that share half of their bits.

Every uniformity statistic is a Pearson chi-square against the uniform expectation, held under the Wilson-Hilferty
approximation of the chi-square quantile at z = 5: df * (1 - 2/(9 df) + 5 sqrt(2/(9 df)))^3.  The bound is derived, not
measured: an ideal sampler passes it with probability 1 - 3e-7 per statistic (for df = 1 and 2 it is looser than the exact
quantile), and with fixed seeds the outcome is deterministic."""
import functools
import math

import numpy as np
import pytest

from helpers import sampler_cases as SC

KEYS = ((0, 0), (5, 3), (2 ** 64 - 1, 2 ** 62 + 3))
STEPS = 200_000
SEEDS = (1, 2 ** 32 + 12345)
SIZES = (2, 3, 4, 5, 7, 11, 16, 17, 33, 64, 65, 97, 256, 257, 1000)
XOR_SIZES = (256, 1024, 4096)
# the four-round form (hb > 8): its first n, where the walk is longest, and the whole of its smallest domain, where its
# known xor excess S / 2^hb = 391 is largest against the statistic's own deviation sqrt(2 df) = 724
WIDE_SIZES = (2 ** 16 + 1, 2 ** 18)


def test_mix32_fixed_points():
    for x, want in ((0, 0), (1, 0x688990C0), (2, 0xD1132181), (0xFFFFFFFF, 0x6768824A), (0x12345678, 0xF5E71C96)):
        assert SC.mix32(x) == want, hex(x)
    x = np.array([0, 1, 2, 0xFFFFFFFF, 0x12345678], dtype=np.uint64)
    assert SC._mix32_np(x).tolist() == [SC.mix32(int(v)) for v in x]


def test_half_bits_fixed_points():
    for n, want in ((1, 1), (2, 1), (4, 1), (5, 2), (16, 2), (17, 3), (64, 3), (65, 4), (256, 4), (257, 5), (2 ** 20, 10),
                    (2 ** 20 + 1, 11), (2 ** 32 + 7, 17), (2 ** 40, 20)):
        assert SC.half_bits(n) == want, n


def test_round_keys_are_distinct_within_a_step_and_between_neighbouring_steps():
    """One key per round and step: no key of steps s..s+63 occurs twice among the rounds of equal parity (rounds of
    different parity mix different halves of the seed and can meet only by chance), also where uint32(step) wraps and at
    the 2^64 end; the vectorised schedule is the scalar one."""
    for seed in (0, 1, 2 ** 32 + 12345, 2 ** 64 - 1):
        for s0 in (0, 2 ** 28 - 32, 2 ** 30 - 32, 2 ** 32 - 32, 2 ** 60 - 32, 2 ** 62 - 32, 2 ** 64 - 64):
            steps = [s0 + k for k in range(64)]
            for n_rounds in (SC.ROUNDS, SC.WIDE_ROUNDS):
                keys = [SC.round_keys(seed, s, n_rounds) for s in steps]
                assert all(len(k) == n_rounds for k in keys)
                assert SC.round_keys_np(seed, np.array(steps, dtype=np.uint64), n_rounds).tolist() == keys
                for parity in (0, 1):
                    flat = [k for ks in keys for k in ks[parity::2]]
                    assert len(set(flat)) == len(flat), (seed, s0, parity, n_rounds)


def test_scalar_and_vectorised_mirror_agree():
    steps = [0, 1, 7, 2 ** 30 - 1, 2 ** 30, 2 ** 32 + 1, 2 ** 62 + 3, 2 ** 64 - 1]
    for n in (1, 2, 3, 4, 5, 16, 17, 64, 65, 97, 257, 1000, 4097, 2 ** 16, 2 ** 16 + 1, 2 ** 20 + 1, 2 ** 32 + 7, 2 ** 40):
        count = min(n, 40)
        for seed in (0, 1, 2 ** 32 + 12345, 2 ** 63 + 11, 2 ** 64 - 1):
            for first in sorted({0, (n - count) // 2, n - count}):
                want = [[SC.index(n, first + i, seed, s) for i in range(count)] for s in steps[:3 if n > 4097 else None]]
                got = SC.indices(n, first, count, seed, steps[:len(want)])
                assert got.dtype == np.int64 and got.tolist() == want, (n, seed, first)
                one = SC.indices(n, first, count, seed, steps[1])
                assert one.shape == (count,) and one.tolist() == want[1]


@pytest.mark.parametrize("seed,step", KEYS)
def test_the_draw_is_a_bijection(seed, step):
    for n in list(range(1, 301)) + [1000, 4097]:
        assert sorted(SC.indices(n, 0, n, seed, step).tolist()) == list(range(n)), n
    for n in WIDE_SIZES:                                        # the four-round form, from its first n on
        assert np.array_equal(np.sort(SC.indices(n, 0, n, seed, step)), np.arange(n)), n


def test_the_round_count_changes_above_65536_rows():
    assert [SC.rounds(n) for n in (1, 17, 4097, 2 ** 16, 2 ** 16 + 1, 2 ** 18, 2 ** 40)] == [10, 10, 10, 10, 4, 4, 4]
    assert [SC.high_bits(n) for n in (16, 17, 32, 33, 2 ** 15, 2 ** 15 + 1, 2 ** 16 + 1, 2 ** 17)] == [2, 2, 2, 3, 7, 8, 9, 9]


def test_a_window_is_a_slice_and_base_is_added_after_the_draw():
    for n in (1, 5, 17, 97, 256, 1000, 4097):
        for seed, step in KEYS:
            whole = SC.indices(n, 0, n, seed, step)
            for first, count in {(0, n), (n // 3, n - n // 3), (n // 3, max(1, n // 5)), (n - 1, 1), (n, 0)}:
                assert np.array_equal(SC.indices(n, first, count, seed, step), whole[first:first + count])
                assert np.array_equal(SC.indices(n, first, count, seed, step, base=10 ** 12 + 7),
                                      whole[first:first + count] + (10 ** 12 + 7))
                assert np.array_equal(SC.indices(n, first, count, seed, step, base=-3), whole[first:first + count] - 3)


# ---- uniformity ----------------------------------------------------------------------------------------------------
def bound(df):
    return df * (1.0 - 2.0 / (9.0 * df) + 5.0 * math.sqrt(2.0 / (9.0 * df))) ** 3


def chi2(counts, total):
    """Pearson statistic of `counts` against `total` spread evenly over the cells."""
    counts = np.asarray(counts, dtype=np.float64)
    assert counts.sum() == total
    e = total / counts.size
    return float(((counts - e) ** 2).sum() / e)


def test_the_bound_is_the_z5_quantile():
    """Against the exact chi-square quantiles at the upper tail 2.8665e-7 (z = 5; by bisection on the regularised
    incomplete gamma function in fp64): the formula lies above each, by 17 % at df = 1, 11 % at df = 2, under 3 % from
    df = 10 and under 0.2 % from df = 100 on."""
    for df, exact, slack in ((1, 26.3376, 0.17), (2, 30.1300, 0.11), (10, 49.8314, 0.03), (100, 187.3257, 0.002),
                             (1000, 1239.8206, 0.0001), (4094, 4562.5459, 0.0001)):
        assert 0.0 < bound(df) / exact - 1.0 < slack, (df, bound(df))


@functools.lru_cache(maxsize=2)
def _draws(n, seed, first, count):
    out = SC.indices(n, first, count, seed, np.arange(STEPS, dtype=np.uint64))
    out.setflags(write=False)
    return out


def _check(stats, n, seed):
    """stats: [(name, statistic, df)].  Prints every figure, then holds each under its bound."""
    bad = []
    for name, x, df in stats:
        print(f"n={n} seed={seed} {name}: chi2={x:.1f} df={df} bound={bound(df):.1f} ratio={x / bound(df):.3f}")
        if not x <= bound(df):
            bad.append((name, round(x, 1), df, round(bound(df), 1)))
    assert not bad, f"n={n} seed={seed}: not uniform in {bad}"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", SIZES + WIDE_SIZES)
def test_rows_drawn_from_a_small_store_are_uniform(n, seed):
    """At the two WIDE_SIZES a cell expects 0.8 to 24 counts; Pearson's statistic of evenly expected cells keeps the mean
    df and the variance 2 df (N - 1)/N at any filling, and over 65 536 cells and more it is normal, as the bound's is."""
    B = min(n, 8)
    d = _draws(n, seed, 0, B)
    p0, p1 = d[:, 0], d[:, 1]
    stats = [("pos0", chi2(np.bincount(p0, minlength=n), STEPS), n - 1)]
    if B < n:
        stats.append(("incl", chi2(np.bincount(d.ravel(), minlength=n), STEPS * B), n - 1))
    assert (p0 != p1).all()
    if n <= 33:                                             # ordered (row at 0, row at 1), the diagonal cannot occur
        table = np.bincount(p0 * n + p1, minlength=n * n).reshape(n, n)
        assert not np.diag(table).any()
        stats.append(("pair", chi2(table[~np.eye(n, dtype=bool)], STEPS), n * (n - 1) - 1))
    else:
        stats.append(("pair", chi2(np.bincount((p1 - p0) % n, minlength=n)[1:], STEPS), n - 2))
    stats.append(("step", chi2(np.bincount((p0[1:] - p0[:-1]) % n, minlength=n), STEPS - 1), n - 1))
    _check(stats, n, seed)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", XOR_SIZES + WIDE_SIZES[1:])
def test_the_xor_of_two_positions_is_uniform(n, seed):
    """Positions (0, 1) and (0, 2^k) for every 2^k < n — (0, 2^hb) differ in the left half alone, where a Feistel network
    of too few rounds leaves the xor of the two images on single values twice as often as it should."""
    a = _draws(n, seed, 0, 2)
    stats = [("xor(0,1)", chi2(np.bincount(a[:, 0] ^ a[:, 1], minlength=n)[1:], STEPS), n - 2)]
    k = 1
    while 2 ** k < n:
        b = SC.indices(n, 2 ** k, 1, seed, np.arange(STEPS, dtype=np.uint64))[:, 0]
        stats.append((f"xor(0,{2 ** k})", chi2(np.bincount(a[:, 0] ^ b, minlength=n)[1:], STEPS), n - 2))
        k += 1
    _check(stats, n, seed)
