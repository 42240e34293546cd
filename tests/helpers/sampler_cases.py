"""Pure-integer restatement of the keyed row sampler (csrc/kernels.hpp: mix32, feistel_index; csrc/porl_api.hip:
feistel_half_bits): row(i) = the image of position i under a Feistel permutation keyed by (seed, step), cycle-walked into
[0, n).  Two forms, chosen by hb = half_bits(n) alone:

  hb <= SMALL_HB (n <= 65 536)  ROUNDS = 10 rounds on the hb low bits and the hb or hb - 1 high bits of a position: the
                                narrower pair of halves where its 2^(2 hb - 1) points already cover n and hb >= 3 (a half
                                of one bit mixes too slowly), so that from 17 rows on fewer than half of the walk's steps
                                leave [0, n).  Counter uint32(step) * 16 + r.
  hb >  SMALL_HB                WIDE_ROUNDS = 4 rounds on 2 hb bits, counter uint32(step) * 4 + r.

A slow scalar form on Python ints and a numpy uint64 form vectorised over positions and steps."""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
ROUNDS = 10                                                 # even: the halves are back in place after the last round
WIDE_ROUNDS = 4
SMALL_HB = 8                                                # the largest hb that takes ROUNDS rounds
MAX_ROWS = 1 << 40                                          # porl_sample_indices / porl_epoch_indices refuse more


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def half_bits(n):
    bits = 1
    while (1 << bits) < n:
        bits += 1
    return max(1, (bits + 1) // 2)


def rounds(n):
    return ROUNDS if half_bits(n) <= SMALL_HB else WIDE_ROUNDS


def high_bits(n):
    """Width of the high half: hb - 1 where 3 <= hb <= SMALL_HB and 2^(2 hb - 1) >= n, else hb."""
    hb = half_bits(n)
    return hb - 1 if 3 <= hb <= SMALL_HB and (1 << (2 * hb - 1)) >= n else hb


def round_keys(seed, step, n_rounds=ROUNDS):
    """ROUNDS keys:      key[r] = mix32(seed half by the parity of r  ^  mix32((uint32(step) * 16 + r, wrapped)  ^  t)),
                         t = mix32(uint32(step >> 28)) ^ uint32(step >> 60) carries the bits of step that the wrap drops.
    WIDE_ROUNDS keys: key[r] = mix32(seed half by the parity of r  ^  mix32(uint32(step) * 4 + r, wrapped)  ^
                         uint32(step >> 30))."""
    assert n_rounds in (ROUNDS, WIDE_ROUNDS)
    seed &= M64
    step &= M64
    half = lambda r: (seed >> 32 if r & 1 else seed) & M32
    if n_rounds == WIDE_ROUNDS:
        return [mix32(half(r) ^ mix32(((step & M32) * 4 + r) & M32) ^ ((step >> 30) & M32)) for r in range(WIDE_ROUNDS)]
    t = mix32((step >> 28) & M32) ^ (step >> 60)
    return [mix32(half(r) ^ mix32((((step & M32) * 16 + r) & M32) ^ t)) for r in range(ROUNDS)]


def index(n, i, seed, step):
    """Row drawn at position i < n of the permutation (seed, step) of [0, n)."""
    assert 0 <= i < n <= MAX_ROWS
    wb, wa = half_bits(n), high_bits(n)
    keys = round_keys(seed, step, rounds(n))
    assert len(keys) % 2 == 0
    x = i
    while True:
        L, R = x >> wb, x & ((1 << wb) - 1)                 # L: wa bits, R: wb bits; each round swaps the two widths
        wl = wa
        for k in keys:
            L, R = R, (L ^ mix32(R ^ k)) & ((1 << wl) - 1)
            wl = wa + wb - wl
        x = (L << wb) | R
        if x < n:
            return x


def _mix32_np(x):
    """mix32 on a uint64 array whose values are < 2^32 (a product of two such stays below 2^64)."""
    m = np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def round_keys_np(seed, steps, n_rounds=ROUNDS):
    """round_keys for a uint64 array of steps: (len(steps), n_rounds) uint64."""
    assert n_rounds in (ROUNDS, WIDE_ROUNDS)
    m = np.uint64(M32)
    steps = np.asarray(steps, dtype=np.uint64)
    seed &= M64
    half = lambda r: np.uint64((seed >> 32 if r & 1 else seed) & M32)
    if n_rounds == WIDE_ROUNDS:
        lo4, top = ((steps & m) * np.uint64(4)) & m, (steps >> np.uint64(30)) & m
        return np.stack([_mix32_np(half(r) ^ _mix32_np((lo4 + np.uint64(r)) & m) ^ top) for r in range(WIDE_ROUNDS)], axis=1)
    t = _mix32_np((steps >> np.uint64(28)) & m) ^ (steps >> np.uint64(60))
    lo16 = ((steps & m) * np.uint64(16)) & m
    return np.stack([_mix32_np(half(r) ^ _mix32_np(((lo16 + np.uint64(r)) & m) ^ t)) for r in range(ROUNDS)], axis=1)


def indices(n, first, count, seed, step, base=0):
    """base + row at positions first..first+count-1, int64: shape (count,) for an int `step`, (len(step), count) for a
    sequence of steps."""
    assert 0 <= first and 0 <= count and first + count <= n <= MAX_ROWS
    scalar = isinstance(step, (int, np.integer))
    steps = np.array([int(step) & M64] if scalar else step, dtype=np.uint64)
    wb, wa = np.uint64(half_bits(n)), np.uint64(high_bits(n))
    mb, ma = np.uint64((1 << int(wb)) - 1), np.uint64((1 << int(wa)) - 1)
    keys = round_keys_np(seed, steps, rounds(n))
    assert keys.shape[1] % 2 == 0
    x = np.broadcast_to(np.arange(first, first + count, dtype=np.uint64), (len(steps), count)).copy()
    todo = np.ones(x.shape, dtype=bool)
    krow = np.broadcast_to(np.arange(len(steps))[:, None], x.shape)
    while todo.any():
        xs, ks = x[todo], keys[krow[todo]]
        L, R = xs >> wb, xs & mb
        for r in range(keys.shape[1]):
            L, R = R, (L ^ _mix32_np(R ^ ks[:, r])) & (mb if r & 1 else ma)
        x[todo] = (L << wb) | R
        todo = x >= np.uint64(n)
    out = x.astype(np.int64) + np.int64(base)
    return out[0] if scalar else out
