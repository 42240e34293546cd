"""The keyed row sampler on the device against its integer host mirror (tests/helpers/sampler_cases.py, whose statistics
tests/test_sampler_host.py checks), bit for bit: engine.sample_indices and engine.epoch_indices over store sizes around
every change of the Feistel half width and of the round count (ten up to 65 536 rows, four above) up to the accepted
maximum of 2^40 rows, with seeds and steps around each bit that either key schedule shifts or wraps, and the two staging kernels that draw for themselves and hand the rows back — the sampled
IQL batch load (idx_out) and the permuted pair load (start_out / goal_out).  The step kernels that draw in place and
report no rows (qnet_gather_kernel, qnet_fused, bcq_mask, the IQN engine) are held to sample_indices by the
sampled-versus-indexed identity tests beside them."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import sampler_cases as SC
from porl_amd import _native as N
from porl_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

SIZES = (1, 2, 3, 4, 5, 16, 17, 64, 65, 255, 256, 257, 1000, 4096, 4097, 65536, 65537, 2 ** 20 + 1, 2 ** 32 + 7, 2 ** 40)
SEEDS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 11, 2 ** 64 - 1)
# around the 32-bit halves of step and its top bits, where uint32(step) * 16 wraps (2^28, the ten-round form up to 65 536
# rows) or uint32(step) * 4 does (2^30, the four-round form above), and the four bits above 2^60
STEPS = (0, 1, 2 ** 30 - 1, 2 ** 30, 2 ** 32 + 1, 2 ** 62 + 3, 2 ** 28 - 1, 2 ** 28, 2 ** 60 + 5)
GRID = [(n, SEEDS[k % len(SEEDS)], STEPS[k % len(STEPS)]) for k, n in enumerate(SIZES)] + \
       [(n, SEEDS[(k + 3) % len(SEEDS)], STEPS[(k + 5) % len(STEPS)]) for k, n in enumerate((5, 17, 65, 257, 4097, 2 ** 32 + 7))] + \
       [(n, SEEDS[(k + 2) % len(SEEDS)], STEPS[2 + k % 4])             # the four-round form at the steps its schedule turns on
        for k, n in enumerate((65537, 2 ** 18, 2 ** 20 + 1, 2 ** 32 + 7, 2 ** 40, 65536, 10 ** 6, 2 ** 36 + 1))]
SENTINEL = -(2 ** 62) - 9
PAD = 5


def test_the_grid_uses_every_seed_and_step():
    assert {s for _, s, _ in GRID} == set(SEEDS) and {t for _, _, t in GRID} == set(STEPS)
    assert [n for n, _, _ in GRID[:len(SIZES)]] == list(SIZES)


def _out(count):
    return torch.full((count + PAD,), SENTINEL, dtype=torch.int64, device=DEV)


def _assert_rows(out, want):
    """out[:len(want)] is the mirror's draw and the tail still holds the sentinel."""
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = out.cpu()
    assert torch.equal(got[:want.numel()], want), (got[:8].tolist(), want[:8].tolist())
    assert bool((got[want.numel():] == SENTINEL).all())


@pytest.mark.parametrize("n,seed,step", GRID)
def test_sample_indices_equals_the_mirror(n, seed, step):
    count, base = min(n, 1000), 10 ** 13 + 3
    out = _out(count)
    assert E.sample_indices(n, count, seed, step, out=out, base=base) is out
    _assert_rows(out, SC.indices(n, 0, count, seed, step, base=base))


@pytest.mark.parametrize("n,seed,step", GRID)
def test_epoch_indices_equals_the_mirror(n, seed, step):
    count, base = min(n, 1000), -12345
    for first in sorted({0, (n - count) // 2, n - count}):
        out = _out(count)
        E.epoch_indices(n, first, count, seed, step, out=out, base=base)
        _assert_rows(out, SC.indices(n, first, count, seed, step, base=base))


@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_the_last_block_of_a_launch_stops_at_count(count):
    n, seed, step = 65537, 2 ** 63 + 11, 2 ** 32 + 1
    out = _out(count)
    E.sample_indices(n, count, seed, step, out=out, base=7)
    _assert_rows(out, SC.indices(n, 0, count, seed, step, base=7))
    out = _out(count)
    E.epoch_indices(n, n - count, count, seed, step, out=out, base=7)
    _assert_rows(out, SC.indices(n, n - count, count, seed, step, base=7))


def test_refused_draws_leave_the_output_untouched():
    out = _out(16)
    for call in (lambda: E.sample_indices(2 ** 40 + 1, 16, 1, 1, out=out),
                 lambda: E.epoch_indices(2 ** 40 + 1, 0, 16, 1, 1, out=out),
                 lambda: E.sample_indices(15, 16, 1, 1, out=out),                  # batch > n_rows
                 lambda: E.epoch_indices(100, 85, 16, 1, 1, out=out),              # first + count > n_rows
                 lambda: E.epoch_indices(100, -1, 16, 1, 1, out=out)):
        with pytest.raises(N.NativeError):
            call()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    E.sample_indices(2 ** 40, 16, 1, 1, out=out)                                    # the maximum itself is accepted
    _assert_rows(out, SC.indices(2 ** 40, 0, 16, 1, 1))


# ---- kernels that draw for themselves and hand the rows back -----------------------------------------------------------
# n_rows = 4^k and 4^k + 1 (the half width changes between them, and at 4^8 the round count), and 2 * 4^k (+ 1) where the
# high half narrows
CONSUMER_SIZES = (4, 5, 16, 17, 32, 33, 64, 65, 256, 257, 4096, 4097, 65536, 65537)
BATCH = 8


@pytest.fixture(scope="module")
def por():
    from porl_amd.agent.por import POR
    torch.manual_seed(0)
    args = SimpleNamespace(state_size=60, hidden_dim=64, n_hidden=2, layer_norm=False, feature_dim=256, action_size=2,
                           max_batch=BATCH)
    return POR(args, 1000, 0.9, 10.0, device=DEV)


@pytest.fixture(scope="module")
def goal_bc():
    from porl_amd.agent import GoalConditionedBC
    torch.manual_seed(0)
    return GoalConditionedBC(20, 2, 3, 1000, hidden_dim=64, n_hidden=2, device=DEV, max_batch=BATCH)


@pytest.mark.parametrize("k,n", list(enumerate(CONSUMER_SIZES)))
def test_the_sampled_batch_load_draws_the_mirrors_rows(por, k, n):
    S, A = 60, 2
    rows = torch.zeros(n, 2 * S + 2 + A, device=DEV)
    rows[:, S] = torch.arange(n, device=DEV, dtype=torch.float32)               # the reward column names the row
    seed, step = SEEDS[k % len(SEEDS)], STEPS[(k + 2) % len(STEPS)]
    for batch in (min(n, BATCH), 1):
        idx = _out(batch)
        por._engine.load_batch_sampled(rows, batch, seed, step, A, False, idx_out=idx[:batch])
        _assert_rows(idx, SC.indices(n, 0, batch, seed, step))


@pytest.mark.parametrize("k,n", list(enumerate(CONSUMER_SIZES)))
def test_the_permuted_pair_load_draws_the_mirrors_rows(goal_bc, k, n):
    S, G, A = 20, 2, 3
    rows = torch.zeros(n, 2 * S + 2 + A, device=DEV)
    seed, step = SEEDS[(k + 1) % len(SEEDS)], STEPS[(k + 4) % len(STEPS)]
    for batch in (min(n, BATCH), 1):
        so, go = _out(batch), _out(batch)
        goal_bc._engine.load_batch_pairs(rows, batch, S, A, 0, G, seed=seed, step=step, start_out=so[:batch], goal_out=go[:batch])
        want = SC.indices(n, 0, batch, seed, step)
        _assert_rows(so, want)
        _assert_rows(go, want)
