"""Shared references of the IQN vector tests (tests/test_iqn_vector_host.py on the CPU, tests/test_iqn_vector_gpu.py on the
device): the keyed fraction stream and the rows head of csrc/iqn_vector.hpp restated in numpy.

The stream, as the header states it:
    key     = sm64(seed ^ TAU_TAG ^ use)             use: 0 acting, 1 tau', 2 tau''
    counter = (draw << 32) | e                        draw < 2^32, e < 2^32
    tau     = float32(sm64(key ^ sm64(counter)) >> 40) * 2^-24
    acting    e = (env_offset + i) * n_tau + j        draw = act-step t
    learning  e = b * n + j                           draw = the learn-draw counter
"""
import numpy as np

TAU_TAG = 0x30C9E7BC03E23535                      # sm64(0x49514E5441554652), "IQNTAUFR"
M64 = (1 << 64) - 1


def sm64(z):
    """splitmix64's increment and finaliser on uint64 arrays (ep_sm64 of csrc/episodes.hpp)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sm64_int(z):
    """The same on one Python integer."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def words(seed, use, draw, first, count):
    """The 64-bit words behind elements [first, first + count) of the stream."""
    assert 0 <= draw < (1 << 32) and 0 <= first and first + count <= (1 << 32) and use in (0, 1, 2)
    key = np.uint64(sm64_int((seed & M64) ^ TAU_TAG ^ use))
    e = np.arange(first, first + count, dtype=np.uint64)
    return sm64(key ^ sm64((np.uint64(draw) << np.uint64(32)) | e))


def taus(seed, use, draw, first, count):
    """Elements [first, first + count) of the stream as float32."""
    top = (words(seed, use, draw, first, count) >> np.uint64(40)).astype(np.float32)      # < 2^24: exact
    return top * np.float32(2.0 ** -24)


def mean_rows_f32(z, n_tau):
    """The rows head's values in fp32: z (n * n_tau, A) -> (n, A), s = 0; s += z[n] for n ascending; s / float32(n_tau)."""
    z = np.asarray(z, dtype=np.float32)
    n, A = z.shape[0] // n_tau, z.shape[1]
    z = z.reshape(n, n_tau, A)
    s = np.zeros((n, A), dtype=np.float32)
    for k in range(n_tau):
        s = s + z[:, k]                               # float32 + float32: one rounding, as the kernel's add
    return s / np.float32(n_tau)


HEAD_K = (1, 15, 16, 17, 64, 65, 256)
HEAD_A = (1, 5, 64)
HEAD_N = 1029                                         # 257 full blocks of four waves and one wave


def head_z(K, A, pad):
    """Random z (HEAD_N * K, ru4(A) + pad) float32 with NaN in the padding columns; the same table for every call."""
    ld = (A + 3) // 4 * 4 + pad
    rng = np.random.default_rng(100000 * K + 100 * A + pad)
    z = np.full((HEAD_N * K, ld), np.nan, dtype=np.float32)
    z[:, :A] = rng.standard_normal((HEAD_N * K, A)).astype(np.float32)
    return z
