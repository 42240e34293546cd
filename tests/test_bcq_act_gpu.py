"""The BCQ-constrained batched act on the device (csrc/bcq_act.hpp): porl_bcq_select over the grid of
tests/helpers/bcq_act_cases.py, and porl_qnet_act_rows_bcq against the two engines' forwards.

Everything is an identity except the mask against the fp64 oracle, which is pinned on the rows where no fp64 probability
lies within MARGIN = 1e-5 of the threshold (the helper's docstring has the rounding count behind it, and the CPU test
asserts that at most 2 % of a case's rows are left out)."""
import functools

import numpy as np
import pytest
import torch

from helpers import bcq_act_cases as BC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 11


@functools.lru_cache(maxsize=None)
def reference(A, n, sigma, threshold):
    """Tables, oracle mask and margin rows of one case: computed once, never written to."""
    q, z = BC.tables(A, n, sigma, threshold)
    want, close = BC.mask_f64(z, threshold), BC.near(z, threshold)
    for x in (q, z, want, close):
        x.setflags(write=False)
    return q, z, want, close


def padded(x, pad):
    """x on the device with `pad` NaN columns behind every row: a row stride above the row width."""
    wide = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, :x.shape[1]] = torch.tensor(x).to(DEV)             # (a copy: the shared reference is read-only)
    return wide[:, :x.shape[1]]


def softmax_mask(z, threshold):
    """porl_softmax_mask on the device logits: BehaviorPolicy.sample's kernel."""
    from porl_amd import _native as N
    out = torch.full((z.shape[0], z.shape[1]), float("nan"), dtype=torch.float32, device=DEV)
    N.check(N.lib().porl_softmax_mask(N.ptr(z), z.stride(0), z.shape[0], z.shape[1], float(threshold), 0, N.ptr(out),
                                      N.current_stream_ptr(z)), "porl_softmax_mask")
    return out


@pytest.mark.parametrize("A,n,sigma", BC.cases())
def test_bcq_select_over_the_grid(A, n, sigma):
    from porl_amd.engine import bcq_select, qnet_select
    for threshold in BC.THRESHOLDS:
        q, z, want, close = reference(A, n, sigma, threshold)
        qd, zd = padded(q, 3), padded(z, 2)
        assert n == 1 or (qd.stride(0) == A + 3 and zd.stride(0) == A + 2)
        mask = torch.full((n, A), float("nan"), dtype=torch.float32, device=DEV)
        out = bcq_select(qd, zd, threshold, 0.0, SEED, 4, env_offset=2, mask=mask)
        assert out.dtype == torch.int64 and out.shape == (n,) and out.device.type == "cuda"
        assert torch.equal(mask.view(torch.int32), softmax_mask(zd, threshold).view(torch.int32)), threshold   # bit for bit
        got_mask = mask.cpu().numpy()
        assert np.array_equal(got_mask[~close], want[~close]), threshold          # the oracle, outside the margin
        pick, _ = BC.select(q, got_mask)
        assert np.array_equal(out.cpu().numpy(), pick), threshold                 # the restated fp32 rule, exactly
        assert torch.equal(out, bcq_select(qd, zd, threshold, 0.0, SEED, 4, env_offset=2)), threshold   # without a mask
        # exploration: the mask is written all the same, and one run equals two runs over the halves
        for eps in (0.3, 1.0):
            m2 = torch.full((n, A), float("nan"), dtype=torch.float32, device=DEV)
            both = bcq_select(qd, zd, threshold, eps, SEED, 4, env_offset=2, mask=m2)
            assert torch.equal(m2.view(torch.int32), mask.view(torch.int32))
            if eps == 1.0 and n >= 255 and A <= 5:
                assert set(both.cpu().numpy().tolist()) == set(range(A))          # every action is explored, allowed or not
            if n >= 2:
                h = n // 2
                assert torch.equal(both[:h], bcq_select(qd[:h], zd[:h], threshold, eps, SEED, 4, env_offset=2))
                assert torch.equal(both[h:], bcq_select(qd[h:], zd[h:], threshold, eps, SEED, 4, env_offset=2 + h))
    # threshold 0 and logits in [-20, 20]: every action is allowed, the actions are qnet_select's
    q, z, _, _ = reference(A, n, sigma, 0.0)
    qd, zd = padded(q, 3), padded(np.clip(z * 4.0, -20.0, 20.0), 2)
    for eps in (0.0, 0.3, 1.0):
        for t, off in ((0, 0), (9, 5)):
            mask = torch.empty(n, A, dtype=torch.float32, device=DEV)
            got = bcq_select(qd, zd, 0.0, eps, SEED, t, env_offset=off, mask=mask)
            assert bool((mask == 1.0).all())
            assert torch.equal(got, qnet_select(qd, eps, SEED, t, env_offset=off)), (eps, t, off)


def make_trainer(tmp_path, q_hidden, max_batch=64, S=22, A=5, threshold=0.2):      # 1 / A: a fresh policy's mask is mixed
    from porl_amd.net.q_network import QNetwork
    from porl_amd.train.bcq_trainer import BCQTrainer
    torch.manual_seed(0)
    return BCQTrainer(S, A, 0.99, device=DEV, batch_size=32, max_batch=max_batch, threshold=threshold, log_dir=str(tmp_path),
                      network=lambda s, a: QNetwork(s, a, list(q_hidden)))


@pytest.mark.parametrize("q_hidden", [(64, 64), (160, 64)])
def test_act_rows_bcq_equals_the_forwards_then_bcq_select(q_hidden, tmp_path):
    """96 robots through engines of max_batch 64: a chunk of 64 and a ragged one of 32; [160, 64] is off the one-launch plan."""
    from porl_amd.engine import bcq_select
    t = make_trainer(tmp_path, q_hidden)
    eng, beh = t._engine, t._behavior_engine
    eng._ensure_bound(); beh._ensure_bound()
    assert eng.cfg.max_batch == beh.cfg.max_batch == 64 and eng.fused == (q_hidden == (64, 64))
    assert list(beh.cfg.hidden[:2]) == [64, 128]
    with torch.no_grad():
        eng.params_tgt.mul_(0.9)                               # a target network that differs (padding stays zero)
    obs = torch.randn(96, 22, device=DEV)
    seen = {}
    for which in (0, 1):
        want_q = torch.cat([eng.forward(obs[:64], which=which), eng.forward(obs[64:], which=which)])
        want_z = torch.cat([beh.forward(obs[:64]), beh.forward(obs[64:])])
        for eps in (0.0, 0.4):
            want_m = torch.empty(96, 5, device=DEV)
            want = bcq_select(want_q, want_z, t.threshold, eps, 21, 6, env_offset=3, mask=want_m)
            tq, tz, mask = (torch.full((96, 5), float("nan"), device=DEV) for _ in range(3))
            got = eng.act_rows_bcq(beh, obs, t.threshold, eps, 21, 6, env_offset=3, q=tq, logits=tz, mask=mask, which=which)
            assert torch.equal(tq, want_q) and torch.equal(tz, want_z), (which, eps)
            assert torch.equal(got, want) and torch.equal(mask, want_m), (which, eps)
        seen[which] = want_q
        assert 0 < float(want_m.mean()) < 1                    # the constraint binds on some actions and not on others
    assert not torch.equal(seen[0], seen[1])                   # the two parameter sets were both exercised
    # the trainer's call: constrained is the new rule at its threshold, unconstrained the engine's act_rows
    assert torch.equal(t.act_rows(obs, 0.4, 21, 6, env_offset=3), eng.act_rows_bcq(beh, obs, t.threshold, 0.4, 21, 6, env_offset=3))
    assert torch.equal(t.act_rows(obs, 0.4, 21, 6, env_offset=3, constrained=False), eng.act_rows(obs, 0.4, 21, 6, env_offset=3))
    assert not torch.equal(t.act_rows(obs, 0.0, 21, 6), t.act_rows(obs, 0.0, 21, 6, constrained=False))


def test_error_paths(tmp_path):
    from porl_amd import _native as N
    from porl_amd.engine import QnetEngine, bcq_select
    t = make_trainer(tmp_path, (64, 64))
    eng, beh = t._engine, t._behavior_engine
    obs = torch.randn(8, 22, device=DEV)
    q, z = torch.randn(8, 5, device=DEV), torch.randn(8, 5, device=DEV)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(N.NativeError, match="threshold"):
            bcq_select(q, z, bad, 0.0, 0, 0)
        with pytest.raises(N.NativeError, match="threshold"):
            eng.act_rows_bcq(beh, obs, bad, 0.0, 0, 0)
    for other in (QnetEngine(21, 5, [64, 128], 64, DEV), QnetEngine(22, 4, [64, 128], 64, DEV)):     # mismatched engines
        with pytest.raises(N.NativeError, match="does not match"):
            eng.act_rows_bcq(other, obs, 0.1, 0.0, 0, 0)
    with pytest.raises(N.NativeError, match="must not be the Q engine"):
        eng.act_rows_bcq(eng, obs, 0.1, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="HIP device"):                        # CPU tensors
        bcq_select(q.cpu(), z.cpu(), 0.1, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="logits"):
        bcq_select(q, z.cpu(), 0.1, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="logits"):
        bcq_select(q, z[:, :4], 0.1, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="mask"):
        bcq_select(q, z, 0.1, 0.0, 0, 0, mask=torch.empty(8, 6, device=DEV))
    with pytest.raises(RuntimeError, match="engine on"):
        eng.act_rows_bcq(beh, obs.cpu(), 0.1, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="logits"):
        eng.act_rows_bcq(beh, obs, 0.1, 0.0, 0, 0, logits=torch.empty(8, 4, device=DEV))
    with pytest.raises(RuntimeError, match="contiguous"):                       # the forward writes whole strides: dense only
        eng.act_rows_bcq(beh, obs, 0.1, 0.0, 0, 0, q=torch.empty(8, 7, device=DEV)[:, 1:6])
