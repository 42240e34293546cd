"""numpy / Python-int restatement of what csrc/per_vector.hpp computes beside the existing kernels: the keyed uniforms of
porl_per_sample_keyed, a sum tree rebuilt from its leaves, and the set of nodes a range fill may write."""
import numpy as np

from helpers.navsim_cases import M64, sm64

TAG_SOURCE = int.from_bytes(b"PERKEYED", "big")           # 0x5045524B45594544
TAG = 0xF08CDF1E9B01AC12                                   # = sm64(TAG_SOURCE), the constant of include/porl_hip.h


def keyed_key(seed):
    return sm64((seed & M64) ^ TAG)


def keyed_u(seed, draw, i):
    """u_i of draw `draw`: (sm64(key ^ sm64((draw << 32) | i)) >> 11) * 2^-53."""
    return float(sm64(keyed_key(seed) ^ sm64(((draw << 32) | i) & M64)) >> 11) * 2.0 ** -53


def keyed_us(seed, draw, batch):
    return np.array([keyed_u(seed, draw, i) for i in range(batch)], dtype=np.float64)


def rebuild(tree, capacity):
    """A copy of `tree` (2*capacity - 1 fp64) with every internal node recomputed from its children, left + right in fp64,
    deepest index first."""
    t = np.array(tree, dtype=np.float64, copy=True)
    assert t.shape == (2 * capacity - 1,)
    for p in range(capacity - 2, -1, -1):
        t[p] = t[2 * p + 1] + t[2 * p + 2]
    return t


def range_nodes(capacity, first_slot, n):
    """Every tree node a fill of slots (first_slot + i) % capacity, i < n, may write: the leaves and, by a leaf-to-root walk
    from each, their ancestors."""
    nodes = set()
    for i in range(n):
        node = (first_slot + i) % capacity + capacity - 1
        nodes.add(node)
        while node != 0:
            node = (node - 1) // 2
            nodes.add(node)
    return nodes


def range_recursion(capacity, first_slot, n):
    """The same set by the range rule: the leaves are one run of tree indices (two when the ring wraps), the parents of a
    run [a, b] are the run [(a - 1) // 2, (b - 1) // 2]."""
    first, end = capacity - 1, first_slot + n
    if n == 0:
        return set()
    runs = [(first + first_slot, first + end - 1)] if end <= capacity else \
        [(first + first_slot, first + capacity - 1), (first, first + end - capacity - 1)]
    nodes = set()
    for a, b in runs:
        nodes.update(range(a, b + 1))
        while a > 0:                                       # b >= a > 0; the run [0, 0] is the root
            a, b = (a - 1) // 2, (b - 1) // 2
            nodes.update(range(a, b + 1))
    return nodes
