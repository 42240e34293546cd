"""IQNTrainer.train_online on the native act and the one-call learn step (csrc/iqn_api.inc, the kernels at the end of
csrc/iqn.hpp): the two fused kernels bit for bit against the launches they replace, learn_indexed against the reference
golden and the fp64 oracle, act_greedy against the oracle's argmax, the loop's semantics on the fast path, the opt-outs,
and the arguments porl_iqn_learn turns down."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, sub
from helpers import iqn_cases as IC
from helpers.online_env import RecordingLogger, ToyEnv
from oracle import iqn_oracle as IO
from porl_amd import _native as N
from porl_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _np_sd(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _refuse(*a, **k):
    raise AssertionError("the native IQN path was left")


def _st(t):
    return N.current_stream_ptr(t)


# -- 1. head kernel ---------------------------------------------------------------------------------------------------
def _head_reference(zc, zo, zt, act, r, d, taus, gamma, kappa):
    """porl_iqn_target + porl_iqn_select + porl_iqn_quantile_huber + porl_iqn_scatter: the launches of learn_on."""
    lib = N.lib()
    B, NP, A = zc.shape
    NPP = zo.shape[1]
    td, na = torch.empty(B, NPP, device=DEV), torch.empty(B, dtype=torch.int64, device=DEV)
    N.check(lib.porl_iqn_target(N.ptr(zo), N.ptr(zt), N.ptr(r), N.ptr(d), gamma, B, NPP, A, N.ptr(td), N.ptr(na), _st(td)))
    cur = torch.empty(B, NP, device=DEV)
    N.check(lib.porl_iqn_select(N.ptr(zc), N.ptr(act), B, NP, A, N.ptr(cur), _st(cur)))
    dcur, row_loss = torch.empty(B, NP, device=DEV), torch.empty(B, device=DEV)
    N.check(lib.porl_iqn_quantile_huber(N.ptr(cur), N.ptr(td), N.ptr(taus), B, NP, NPP, kappa, N.ptr(dcur), N.ptr(row_loss), _st(cur)))
    dz = torch.empty(B, NP, A, device=DEV)
    N.check(lib.porl_iqn_scatter(N.ptr(dcur), N.ptr(act), B, NP, A, N.ptr(dz), _st(dz)))
    return dz, row_loss, na


def _head(zc, zo, zt, act, r, d, taus, gamma, kappa, ld=None):
    B, NP, A = zc.shape
    NPP = zo.shape[1]
    ld = A if ld is None else ld

    def rows(z):                                           # (B, n, A) -> (B * n, ld) rows, padding filled with a sentinel
        out = torch.full((z.shape[0] * z.shape[1], ld), 7.5, device=DEV)
        out[:, :A] = z.reshape(-1, A)
        return out
    dz = torch.full((B * NP, ld), -3.0, device=DEV)
    row_loss, na = torch.empty(B, device=DEV), torch.empty(B, dtype=torch.int64, device=DEV)
    zc, zo, zt = rows(zc), rows(zo), rows(zt)
    N.check(N.lib().porl_iqn_head(N.ptr(zc), N.ptr(zo), N.ptr(zt), ld, N.ptr(act), N.ptr(r), N.ptr(d),
                                  N.ptr(taus), B, NP, NPP, A, gamma, kappa, N.ptr(dz), N.ptr(row_loss), N.ptr(na), _st(dz)),
            "porl_iqn_head")
    return dz, row_loss, na


@pytest.mark.parametrize("kappa", [0.5, 1.0])
@pytest.mark.parametrize("B,NP,NPP,A", [(6, 4, 4, 3), (37, 3, 5, 2), (1, 1, 1, 3), (3, 70, 9, 4),
                                        # a second pass of the Bellman-target loop; both limits; a third pass with one row
                                        (5, 3, 65, 33), (2, 256, 256, 64), (4, 1, 129, 64)])
def test_head_kernel_has_the_bits_of_the_four_launches_it_replaces(B, NP, NPP, A, kappa):
    g = torch.Generator().manual_seed(100 * B + NP)
    zc, zt = torch.randn(B, NP, A, generator=g), torch.randn(B, NPP, A, generator=g)
    zo = torch.randn(B, NPP, A, generator=g)
    d = (torch.rand(B, generator=g) < 0.3).float()
    if (B, NP) == (6, 4):                                  # the tie / mean / terminal rows of test_target_kernel_picks_the_first_maximum...
        zo = torch.zeros(B, NPP, A)
        zo[0, :, 2] = 1.0
        zo[1, :, 1] = 1.0
        zo[1, :, 2] = 1.0                                  # tie between actions 1 and 2: the first wins
        zo[2, 0, 0], zo[2, 1, 1] = 4.0, 5.0                # the choice is on the tau-MEAN
        d = torch.tensor([0, 0, 0, 1, 0, 1], dtype=torch.float32)
    r = 2.0 * torch.randn(B, generator=g)
    act = torch.randint(0, A, (B,), generator=g)
    taus = torch.rand(B, NP, generator=g)
    args = [x.to(DEV).contiguous() for x in (zc, zo, zt, act, r, d, taus)]
    want_dz, want_loss, want_na = _head_reference(*args, 0.9, kappa)
    if (B, NP) == (6, 4):
        assert want_na.tolist()[:3] == [2, 1, 1]
    assert bool(torch.isfinite(want_loss).all()) and float(want_dz.abs().max()) > 0
    for ld in (A, (A + 3) // 4 * 4 + 4):
        dz, loss, na = _head(*args, 0.9, kappa, ld=ld)
        assert torch.equal(na, want_na)
        assert torch.equal(loss, want_loss)
        assert torch.equal(dz[:, :A].reshape(B, NP, A), want_dz)
        assert not bool(dz[:, A:].any())                   # the padding columns of the gradient rows are zero
    # a row with an action outside 0..A-1: NaN row loss, no gradient; the other rows are untouched
    bad = args[3].clone()
    bad[B // 2] = A
    args[3] = bad
    want_dz, want_loss, _ = _head_reference(*args, 0.9, kappa)
    dz, loss, _ = _head(*args, 0.9, kappa)
    ok = torch.arange(B, device=DEV) != B // 2
    assert bool(torch.isnan(loss[B // 2])) and bool(torch.isnan(want_loss[B // 2]))
    assert torch.equal(loss[ok], want_loss[ok]) and torch.equal(dz.reshape(B, NP, A), want_dz)
    assert not bool(dz.reshape(B, NP, A)[B // 2].any())


# -- 2. mix kernel ----------------------------------------------------------------------------------------------------
def _mix_reference(feat, taus, We, be):
    from porl_amd.net.iqn_network import cos_embed
    B, H = feat.shape
    n, Ed = taus.shape[1], We.shape[1]
    ce = cos_embed(taus, Ed)                                                            # porl_iqn_cos_embed
    emb = torch.empty(B * n, H, device=DEV)
    E.gemm_f32(0, ce, We, B * n, H, Ed, Ed, Ed, emb, H, bias=be)                         # porl_gemm_f32, bias, no activation
    out = torch.empty_like(emb)
    N.check(N.lib().porl_iqn_hadamard(N.ptr(feat), H, N.ptr(emb), B, n, H, N.ptr(out), _st(out)), "porl_iqn_hadamard")
    return out, emb


@pytest.mark.parametrize("nprob", [1, 3])
@pytest.mark.parametrize("B,n,Ed,H", [(33, 5, 16, 48), (8, 1, 10, 30), (2, 9, 8, 4), (64, 8, 64, 512),
                                      # full LDS panels with a one-column block; E % 8 = 7; E = 17 on unaligned rows
                                      (3, 2, 128, 65), (2, 3, 127, 64), (5, 7, 17, 30)])
def test_mix_kernel_has_the_bits_of_cos_embed_gemm_hadamard(B, n, Ed, H, nprob):
    g = torch.Generator().manual_seed(B + H + nprob)
    probs, keep, want = (N.IqnMixProb * nprob)(), [], []
    for k in range(nprob):
        nk = n if k == 0 else n + 1                        # the problems of one launch need not have equal row counts
        feat = torch.randn(B, H, generator=g).to(DEV)
        taus = torch.rand(B, nk, generator=g).to(DEV)
        We = (torch.randn(H, Ed, generator=g) / Ed ** 0.5).to(DEV)
        be = torch.randn(H, generator=g).to(DEV)
        out = torch.full((B * nk, H), 9.0, device=DEV)
        emb = torch.full((B * nk, H), 9.0, device=DEV) if k == 0 else None
        probs[k] = N.IqnMixProb(feat.data_ptr(), H, taus.data_ptr(), We.data_ptr(), Ed, be.data_ptr(), out.data_ptr(), H,
                                None if emb is None else emb.data_ptr(), B, nk)
        keep.append((feat, taus, We, be, out, emb))
        want.append(_mix_reference(feat, taus, We, be))
    N.check(N.lib().porl_iqn_mix(nprob, probs, Ed, H, _st(keep[0][0])), "porl_iqn_mix")
    for (feat, taus, We, be, out, emb), (want_out, want_emb) in zip(keep, want):
        assert torch.equal(out, want_out)
        if emb is not None:
            assert torch.equal(emb, want_emb)


# -- 3. reference golden ----------------------------------------------------------------------------------------------
def _golden():
    z = np.load(os.path.join(GOLDEN, "iqn_s9_a5.npz"), allow_pickle=False)
    return z, tuple(int(v) for v in z["meta"][:8])


def _golden_trainer(z, S, A, Ed, H, B, NP, NPP, **kw):
    from porl_amd.train.iqn_trainer import IQNTrainer
    t = IQNTrainer(S, A, gamma=float(z["gamma"]), device=DEV, learning_rate=float(z["lr"]), batch_size=B,
                   kappa=float(z["kappa"]), embedding_dim=Ed, hidden_size=H, num_quantiles_n_prime_loss=NP,
                   num_quantiles_n_double_prime_loss=NPP, **kw)
    t.q_network.load_state_dict({k: torch.from_numpy(v) for k, v in sub(z, "init/").items()})
    t.target_network.load_state_dict({k: torch.from_numpy(v) for k, v in sub(z, "init_target/").items()})
    return t


def _no_autograd_path(monkeypatch, t):
    from porl_amd.net.iqn_network import IQNNetwork, SelectAction
    monkeypatch.setattr(t, "learn_on", _refuse)
    monkeypatch.setattr(IQNNetwork, "forward", _refuse)
    monkeypatch.setattr(SelectAction, "apply", _refuse)


def test_learn_indexed_matches_reference_golden(monkeypatch):
    z, (S, A, Ed, H, B, K, NP, NPP) = _golden()
    t = _golden_trainer(z, S, A, Ed, H, B, NP, NPP)
    for i in range(K * B):
        t.replay_buffer.push(z["states"][i], int(z["actions"][i]), float(z["rewards"][i]), z["next_states"][i], bool(z["dones"][i]))
    _no_autograd_path(monkeypatch, t)
    for k in range(K):
        loss = t.learn_indexed(torch.arange(k * B, (k + 1) * B, device=DEV), torch.from_numpy(z["taus_prime"][k]),
                               torch.from_numpy(z["taus_double_prime"][k]))
        assert isinstance(loss, float)
        np.testing.assert_allclose(loss, z["loss"][k], rtol=1e-5)
    assert t.optimizer.step_count == K
    for k, ref in sub(z, "final/").items():
        np.testing.assert_allclose(_np_sd(t.q_network)[k], ref, atol=1e-5, err_msg=k)
    for k, ref in sub(z, "init_target/").items():          # the target network is untouched until sync_target
        np.testing.assert_array_equal(_np_sd(t.target_network)[k], ref)
    t.sync_target()
    for k, v in _np_sd(t.q_network).items():
        np.testing.assert_array_equal(_np_sd(t.target_network)[k], v)


def test_learn_indexed_raises_learn_ons_index_error():
    z, (S, A, Ed, H, B, K, NP, NPP) = _golden()
    t = _golden_trainer(z, S, A, Ed, H, B, NP, NPP)
    for i in range(B):
        t.replay_buffer.push(z["states"][i], A if i == 3 else int(z["actions"][i]), float(z["rewards"][i]), z["next_states"][i],
                             bool(z["dones"][i]))
    with pytest.raises(IndexError):
        t.learn_indexed(torch.arange(B, device=DEV))
    t.async_losses = True
    stats = t.learn_indexed(torch.arange(B, device=DEV))
    assert isinstance(stats, torch.Tensor) and stats.shape == (3,) and stats.device.type == "cuda"


# -- 4. fp64 oracle ---------------------------------------------------------------------------------------------------
def _flat_views(t, flat):
    out, off = {}, 0
    for k, p in t.q_network.named_parameters():
        out[k] = flat[off:off + p.numel()].view_as(p).cpu().numpy().astype(np.float64)
        off += (p.numel() + 3) // 4 * 4
    return out


def _against_oracle(t, o, got, want, norm, small, lr, P_before):
    """The assertions of test_iqn_gpu.py:test_gradients_and_loss_match_the_fp64_oracle on one step."""
    np.testing.assert_allclose(got, want, rtol=1e-5)
    np.testing.assert_allclose(norm, o.grad_norm, rtol=1e-5)
    for k, p_ in t.q_network.named_parameters():
        g, want_g = p_.grad.cpu().numpy().astype(np.float64), o.G[k]
        if small:
            assert np.abs(g - want_g).max() <= 1e-5 * np.abs(want_g).max() + 1e-12, (k, np.abs(g - want_g).max(), np.abs(want_g).max())
        else:                                              # the ReLU-mask flips of that test's large size: relative 2-norm
            assert np.linalg.norm(g - want_g) <= 5e-3 * np.linalg.norm(want_g), (k, np.linalg.norm(g - want_g), np.linalg.norm(want_g))
    P1 = _np_sd(t.q_network)
    for k in IO.NAMES:
        d = np.abs(P1[k] - o.P[k])
        sensitive = np.abs(o.G[k]) < (1e-6 if small else 2e-5)
        assert d.max() <= 2 * lr * 1.001 and (d[~sensitive] <= 2e-6).all(), (k, d.max(), d[~sensitive].max())


@pytest.mark.parametrize("B,H,Ed,NP,NPP,A,max_norm", [(64, 512, 64, 8, 8, 4, 10.0), (37, 40, 10, 3, 5, 2, 10.0),
                                                      (1, 24, 8, 1, 1, 3, 10.0), (37, 40, 10, 3, 5, 2, 0.05)])
def test_learn_indexed_matches_the_fp64_oracle_and_shares_its_state_with_learn_on(B, H, Ed, NP, NPP, A, max_norm):
    """One native step from the oracle's state, then one learn_on step on the same trainer against an oracle step from
    the state the native step left (parameters AND Adam moments): the two paths work on one set of buffers.  Bounds: those
    of test_gradients_and_loss_match_the_fp64_oracle; the default size (64 x 8 rows of 512) is past that test's
    B * N' * H < 100 000 switch, so its gradients are held to the relative 2-norm form that test uses at its large size."""
    from porl_amd.train.iqn_trainer import IQNTrainer
    S, lr = 13, 1e-3
    small = B * NP * H < 100_000
    rng = np.random.default_rng(B + H)
    torch.manual_seed(5)
    t = IQNTrainer(S, A, gamma=0.95, device=DEV, learning_rate=lr, batch_size=B, kappa=0.5, embedding_dim=Ed, hidden_size=H,
                   num_quantiles_n_prime_loss=NP, num_quantiles_n_double_prime_loss=NPP, max_norm=max_norm)
    with torch.no_grad():
        t._target.flat.add_(0.05 * torch.randn_like(t._target.flat))
    P0, T0 = _np_sd(t.q_network), _np_sd(t.target_network)

    wide = 32.0 if max_norm < 1.0 else 1.0                 # states wide enough for a gradient norm past max_norm

    def batch():
        st, ns = (wide * rng.standard_normal((B, S))).astype(np.float32), (wide * rng.standard_normal((B, S))).astype(np.float32)
        return (st, rng.integers(0, A, B), (2.0 * rng.standard_normal(B)).astype(np.float32), ns,
                (rng.random(B) < 0.2).astype(np.float32), rng.random((B, NP)).astype(np.float32),
                rng.random((B, NPP)).astype(np.float32))
    st, ac, rw, ns, dn, tp, tpp = batch()
    for i in range(B):
        t.replay_buffer.push(st[i], int(ac[i]), float(rw[i]), ns[i], bool(dn[i]))
    o = IO.IqnOracle(P0, T0, gamma=0.95, kappa=0.5, lr=lr, max_norm=max_norm)
    want = o.learn(st, ac, rw, ns, dn, tp, tpp)
    got = t.learn_indexed(torch.arange(B, device=DEV), torch.from_numpy(tp), torch.from_numpy(tpp))
    stats = t._iqn.stats.cpu().numpy()
    assert stats[0] == np.float32(got)
    if max_norm < 1.0:
        assert o.grad_norm > 2 * max_norm and stats[2] < 0.5          # the clip coefficient is well below 1 ...
        np.testing.assert_allclose(stats[2], max_norm / (o.grad_norm + 1e-6), rtol=1e-5)
    else:
        assert stats[2] == 1.0
    _against_oracle(t, o, got, want, stats[1], small, lr, P0)
    for k in IO.NAMES:
        np.testing.assert_array_equal(_np_sd(t.target_network)[k], T0[k])
    # second step through learn_on, from the state the native step left behind
    o2 = IO.IqnOracle(_np_sd(t.q_network), T0, gamma=0.95, kappa=0.5, lr=lr, max_norm=max_norm)
    o2.m, o2.v, o2.t = _flat_views(t, t.optimizer.exp_avg), _flat_views(t, t.optimizer.exp_avg_sq), 1
    assert any(np.abs(v).max() > 0 for v in o2.v.values())
    st, ac, rw, ns, dn, tp, tpp = batch()
    want = o2.learn(st, ac, rw, ns, dn, tp, tpp)
    got = t.learn_on(*(torch.from_numpy(a) for a in (st, ac, rw, ns, dn)), taus_prime=torch.from_numpy(tp),
                     taus_double_prime=torch.from_numpy(tpp))
    assert t.optimizer.step_count == 2
    _against_oracle(t, o2, got, want, float(t.optimizer._clip[0]), small, lr, None)


# -- 5. act -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,n_policy", IC.ACT_CASES)
def test_act_greedy_is_the_oracles_argmax(H, n_policy, monkeypatch):
    from porl_amd.train.iqn_trainer import IQNTrainer
    P, states, taus, want, keep = IC.act_case(H, n_policy)
    assert keep.sum() >= 0.9 * len(keep)
    t = IQNTrainer(IC.ACT_S, IC.ACT_A, 0.99, device=DEV, embedding_dim=IC.ACT_E, hidden_size=H,
                   num_quantiles_n_policy=n_policy, buffer_size=64)
    t.q_network.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    for s in states:
        t.replay_buffer.push(s, 0, 0.0, s, False)
    _no_autograd_path(monkeypatch, t)
    tt = torch.from_numpy(taus).to(DEV)
    inline = np.array([t.act_greedy(state=states[i], taus=tt[i:i + 1]) for i in range(len(states))])
    rows = np.array([t.act_greedy(row=i, taus=tt[i:i + 1]) for i in range(len(states))])
    np.testing.assert_array_equal(inline[keep], want[keep])
    np.testing.assert_array_equal(rows[keep], want[keep])
    a = t.act_greedy(state=states[0])                      # fractions drawn as select_action draws them
    assert 0 <= a < IC.ACT_A
    with pytest.raises(ValueError):
        t.act_greedy()


# -- 6. loop ----------------------------------------------------------------------------------------------------------
class _CountingEnv(ToyEnv):
    def reset(self, seed=None):
        self.ep_len = getattr(self, "ep_len", []) + [0]
        return super().reset(seed)

    def step(self, action):
        self.ep_len[-1] += 1
        return super().step(action)


def _loop_trainer(cls=None, **kw):
    from porl_amd.train.iqn_trainer import IQNTrainer
    args = dict(gamma=0.99, epsilon=0.5, epsilon_decay=1.0, update_target_freq=2, device=DEV, hidden_size=32, embedding_dim=16,
                batch_size=16, num_quantiles_n_prime_loss=4, num_quantiles_n_double_prime_loss=4, num_quantiles_n_policy=8,
                transition_learning_step=20)
    args.update(kw)
    t = (cls or IQNTrainer)(8, 4, **args)
    t.logger = RecordingLogger()
    return t


def _fast_only(t):
    t.select_action = t.learn = t.learn_on = _refuse
    t.replay_buffer.push = t.replay_buffer.sample = _refuse


def test_train_online_runs_on_the_native_act_and_learn_step():
    t = _loop_trainer()
    _fast_only(t)
    env = _CountingEnv(seed=4)
    np.random.seed(2)
    torch.manual_seed(2)
    greedy = []
    orig_act = t._act
    t._act = lambda *a, **k: (greedy.append(k.get("n_stats", 0)), orig_act(*a, **k))[1]
    rewards = _quiet(t.train_online, env, num_episodes=3, max_steps=30)
    assert len(rewards) == 3 and env.closed
    calls, want, n, j = t.logger.calls, [], 0, 0
    for ep, steps in enumerate(env.ep_len):                # the plain loop's call order (online.run)
        for step in range(steps):
            n += 1
            want.append(("log_step", ep, step, None))
            if n >= 20:
                want.append(("log_step", ep, step, "loss"))
        want.append(("log_episode", ep))
    want.append(("close",))
    got = [c[:3] + (None if c[4] is None else "loss",) if c[0] == "log_step" else c[:2] for c in calls]
    assert got == want
    losses = [c[4] for c in calls if c[0] == "log_step" and c[4] is not None]
    assert len(losses) == n - 19 > 20 and all(isinstance(v, float) for v in losses) and np.isfinite(losses).all()
    assert t.optimizer.step_count == len(losses)
    # both routes of the deferred loss were taken: read from the act record (a greedy step followed the learn step) and
    # parked in the device log (an exploring step followed it)
    assert 0 < sum(greedy) < len(losses)
    assert len(set(losses)) == len(losses)                 # every step's own loss, none repeated or dropped
    assert len(t.replay_buffer) == n


def test_async_losses_reach_the_logger_as_the_statistics_view():
    t = _loop_trainer()
    _fast_only(t)
    t.async_losses = True
    np.random.seed(2)
    _quiet(t.train_online, _CountingEnv(seed=4), num_episodes=3, max_steps=30)
    losses = [c[4] for c in t.logger.calls if c[0] == "log_step" and c[4] is not None]
    assert losses and all(isinstance(v, torch.Tensor) and v.device.type == "cuda" and v.shape == (3,) for v in losses)
    assert all(v.data_ptr() == t._iqn.stats.data_ptr() for v in losses)


def test_exploring_run_draws_what_the_plain_loop_draws():
    """epsilon = 1: the fast loop and the plain loop (a subclass that overrides learn_on opts out) consume the numpy and
    the device generator alike, and their first learn step — same weights, same minibatch, same fractions — agrees."""
    from porl_amd.train.iqn_trainer import IQNTrainer

    class Plain(IQNTrainer):
        def learn_on(self, *a, **k):
            return super().learn_on(*a, **k)
    a = _loop_trainer(epsilon=1.0)
    b = _loop_trainer(Plain, epsilon=1.0)
    b.q_network.load_state_dict(a.q_network.state_dict())
    b.sync_target()
    _fast_only(a)
    end = []
    for t in (a, b):
        np.random.seed(7)
        torch.manual_seed(7)
        _quiet(t.train_online, _CountingEnv(seed=4), num_episodes=3, max_steps=30)
        end.append((np.random.get_state(), torch.cuda.get_rng_state(DEV)))
    (na, ta), (nb, tb) = end
    assert na[0] == nb[0] and np.array_equal(na[1], nb[1]) and na[2:] == nb[2:]
    assert torch.equal(ta, tb)
    la, lb = ([c[4] for c in t.logger.calls if c[0] == "log_step" and c[4] is not None] for t in (a, b))
    assert len(la) == len(lb) > 5 and a.optimizer.step_count == b.optimizer.step_count == len(la)
    np.testing.assert_allclose(la[0], lb[0], rtol=1e-5)


# -- 7. opt-outs ------------------------------------------------------------------------------------------------------
def _count_learn_on(t):
    n, orig = [0], t.learn_on

    def counting(*a, **k):
        n[0] += 1
        return orig(*a, **k)
    t.learn_on = counting
    np.random.seed(1)
    _quiet(t.train_online, ToyEnv(seed=4), num_episodes=8, max_steps=30)
    losses = [c[4] for c in t.logger.calls if c[0] == "log_step" and c[4] is not None]
    assert len(losses) > 5 and np.isfinite(losses).all()
    return n[0], len(losses)


def test_overrides_and_foreign_parts_keep_the_plain_loop():
    from porl_amd.buffer.replay_buffer import ReplayBuffer
    from porl_amd.train import online
    from porl_amd.train.iqn_trainer import IQNTrainer

    class OwnLearn(IQNTrainer):
        def learn(self):
            return super().learn()

    class OwnLearnOn(IQNTrainer):
        def learn_on(self, *a, **k):
            return super().learn_on(*a, **k)

    class OwnSelect(IQNTrainer):
        def select_action(self, state):
            return super().select_action(state)

    class OtherBuffer(ReplayBuffer):
        pass
    t = _loop_trainer()
    assert online.fast_iqn_ok(t)
    assert _count_learn_on(t)[0] == 0                      # the fast path never calls learn_on
    for t in (_loop_trainer(OwnLearn), _loop_trainer(OwnLearnOn), _loop_trainer(OwnSelect),
              _loop_trainer(replay_buffer=OtherBuffer(1000, (8,), DEV)), _loop_trainer(embedding_dim=129)):
        assert not online.fast_iqn_ok(t)
        calls, steps = _count_learn_on(t)
        assert calls == steps > 0


# -- 8. rejected arguments --------------------------------------------------------------------------------------------
def test_learn_names_the_argument_it_rejects():
    t = _loop_trainer()
    for tr in range(32):
        t.replay_buffer.push(np.zeros(8, np.float32), tr % 4, 0.0, np.zeros(8, np.float32), False)
    t.replay_buffer._sync_mirror()
    eng, m = t._native_engine(), t.replay_buffer._mirror
    before = t.optimizer.flat.clone()
    idx = torch.arange(16, device=DEV)
    tp, tpp = torch.rand(16, 4, device=DEV), torch.rand(16, 4, device=DEV)
    lib, p = N.lib(), N.ptr

    def call(batch=16, s_rs=8, n_rs=8, n_cur=4, n_tgt=4, step=1, null=None, hp=True):
        hyper = eng.hyper(0.99, 1.0, 10.0, step, 5e-4)
        a = dict(states=p(m["states"]), actions=p(m["actions"]), rewards=p(m["rewards"]), next_states=p(m["next_states"]),
                 dones=p(m["dones"]), taus_prime=p(tp), taus_dprime=p(tpp))
        if null:
            a[null] = None
        return lib.porl_iqn_learn(eng._h, a["states"], s_rs, a["actions"], a["rewards"], a["next_states"], n_rs, a["dones"],
                                  p(idx), batch, a["taus_prime"], n_cur, a["taus_dprime"], n_tgt,
                                  C.byref(hyper) if hp else None, N.current_stream_ptr(DEV))

    def rejected(rc, match):
        assert rc != 0
        msg = lib.porl_last_error().decode()
        assert match in msg, msg
    rejected(call(batch=0), "batch 0")
    rejected(call(batch=eng.cfg.max_batch + 1), "batch %d" % (eng.cfg.max_batch + 1))
    rejected(call(s_rs=7), "s_rs 7")
    rejected(call(n_rs=7), "n_rs 7")
    rejected(call(n_cur=eng.cfg.max_tau + 1), "n_cur")
    rejected(call(n_tgt=eng.cfg.max_tau + 1), "n_tgt")
    rejected(call(n_cur=0), "n_cur")
    rejected(call(step=0), "step 0")
    rejected(call(hp=False), "null hp")
    for name in ("states", "actions", "rewards", "next_states", "dones", "taus_prime", "taus_dprime"):
        rejected(call(null=name), "null " + name)
    torch.cuda.synchronize()
    assert torch.equal(t.optimizer.flat, before)           # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(t.optimizer.flat, before)
    with pytest.raises(N.NativeError, match="max_tau"):
        E.IqnEngine(8, 4, 16, 32, 16, 257, DEV)
