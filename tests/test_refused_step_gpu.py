"""A learn call the host layer refuses leaves the optimizer where it was: the Adam step number advances only after the
native call that used it (cql_trainer._FlatAdam.hyper and `step_count = hp.step`), so step number, parameters and moments
stay together.  One case per trainer family, at the smallest shape (S=8, A=4, hidden [16], batch 4 on an engine of
max_batch 4); each first takes one good step, so the state that must survive the refusal is not all zeros.  Every refusal
happens before a launch."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
S, A, B, ROWS = 8, 4, 4, 12


def _rows(seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(S).astype(np.float32), int(rng.integers(A)), float(rng.standard_normal()),
             rng.standard_normal(S).astype(np.float32), bool(rng.random() < 0.25)) for _ in range(ROWS)]


def _buffer():
    from porl_amd.buffer.replay_buffer import ReplayBuffer
    rb = ReplayBuffer(ROWS, (S,), DEV)
    for row in _rows():
        rb.push(*row)
    rb._sync_mirror()
    return rb


def _idx(n):
    return torch.arange(n, dtype=torch.int64, device=DEV)


def _qnet(cls, **kw):
    from porl_amd.net.q_network import QNetwork
    torch.manual_seed(0)
    return cls(S, A, 0.9, device=DEV, network=lambda s, a: QNetwork(s, a, [16]), batch_size=B, max_batch=B,
               replay_buffer=_buffer(), **kw)


def _qnet_state(*engines):
    return lambda: [getattr(e, k) for e in engines for k in ("params", "params_tgt", "adam_m", "adam_v")]


def cql():
    from porl_amd.train.cql_trainer import CQLTrainer
    t = _qnet(CQLTrainer, alpha=1.0)
    return t.optimizer, _qnet_state(t._engine), lambda n: t._learn_rows(_idx(n))


def ddqn():
    from porl_amd.train.dqn_trainer import DDQNTrainer
    t = _qnet(DDQNTrainer)
    return t.optimizer, _qnet_state(t._engine), lambda n: t.learn_on(*t.replay_buffer.gather_device(_idx(n)))


def per():
    from porl_amd.train.dqn_per_trainer import PERTrainer
    t = _qnet(PERTrainer, capacity=16)
    for row in _rows():
        t.memory.add(1.0, *row)
    random.seed(0)

    def learn(n):
        t.batch_size = n
        return t.learn()
    return t.optimizer, _qnet_state(t._engine), learn


def bcq():
    from porl_amd.policy.bcq import bcq_learn_rows
    from porl_amd.train.bcq_trainer import BCQTrainer
    t = _qnet(BCQTrainer)
    return t.optimizer, _qnet_state(t._engine, t._behavior_engine), lambda n: bcq_learn_rows(t, _idx(n))


def qrdqn():
    from porl_amd.train.qr_dqn_trainer import QRDQNTrainer
    torch.manual_seed(0)
    t = QRDQNTrainer(S, A, 0.9, device=DEV, network_hidden_sizes=[16], num_quantiles=5, batch_size=B, max_batch=B,
                     replay_buffer=_buffer())
    return t.optimizer, _qnet_state(t._engine), lambda n: t.learn_indexed(_idx(n))


def iqn():
    from porl_amd.train.iqn_trainer import IQNTrainer
    torch.manual_seed(0)
    t = IQNTrainer(S, A, 0.9, device=DEV, batch_size=B, embedding_dim=16, hidden_size=32, num_quantiles_n_prime_loss=4,
                   num_quantiles_n_double_prime_loss=4, replay_buffer=_buffer())
    o = t.optimizer

    def learn(n):                                          # n == B: learn()'s own draws; else fractions of n rows for B rows
        tp = None if n == B else torch.rand(n, 4, device=DEV)
        return t.learn_indexed(_idx(B), taus_prime=tp)
    return o, (lambda: [o.flat, t._target.flat, o.exp_avg, o.exp_avg_sq]), learn


@pytest.mark.parametrize("make", [cql, ddqn, per, bcq, qrdqn, iqn])
def test_a_refused_call_leaves_step_count_parameters_and_moments(make):
    opt, state, learn = make()
    learn(B)                                               # one good step: moments and step number are no longer zero
    torch.cuda.synchronize()
    assert opt.step_count == 1
    before = [x.clone() for x in state()]
    assert all(float(x.abs().max()) > 0 for x in before[:4])          # (BCQ's behaviour engine, listed after, has not stepped)
    with pytest.raises(RuntimeError):
        learn(B + 1)                                       # 5 rows on an engine of max_batch 4 / fractions of 5 rows for 4
    torch.cuda.synchronize()
    assert opt.step_count == 1
    for x, y in zip(state(), before):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    learn(B)                                               # and the next good step is Adam step 2
    torch.cuda.synchronize()
    assert opt.step_count == 2
    assert not torch.equal(state()[0], before[0])
