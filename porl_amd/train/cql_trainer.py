"""CQL trainer — drop-in for the hot path of /root/reference/src/porl/train/cql_trainer.py (+ the pieces of
dqn_trainer.py it inherits): `learn()`, `compute_cql_penalty`, `train_offline`, `get_action`,
`select_action`, with `q_network`, `target_network`, `optimizer`, `replay_buffer`, `batch_size`, `gamma`,
`alpha`, `action_size`, `device` attributes.

The reference's constructor is broken upstream (it forwards 10 positionals to an 11-positional base,
SURVEY.md §2.1); this one accepts the keyword call of scripts/train_cql.py:18-29 and behaves as evidently
intended (`learning_rate` defaults to the hard-coded 5e-4 of dqn_trainer.py:71).

`learn()` = sample (host index stream identical to the reference under the same numpy seed, gather on the
device) + one fused device update: target forward, online forward, TD + CQL(H) penalty, backward, Adam —
hand-written gfx950 kernels behind `porl_qnet_*` (include/porl_hip.h), reached through engine.QnetEngine (the ctypes
layer, with the one replay-array check `engine.replay_args`).

Host bookkeeping every Q-learning trainer shares lives here: `_FlatAdam.hyper` builds the hyper-parameters of the NEXT
Adam step without advancing anything — a caller makes its native call(s) and then sets `step_count = hp.step`, so a
refused call leaves the optimizer where it was; `read_losses` is the one read-back of the step statistics, `checked_loss`
the reference's IndexError for an action outside 0..A-1, `learn_minibatch` the step on an explicit minibatch.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import engine as E
from ..buffer.replay_buffer import ReplayBuffer
from ..engine import QnetEngine                                     # (tests and scripts import it from here)
from ..net.q_network import DuelingQNetwork, QNetwork
from ..parallel import GradExchange
from ..utils.logger import Logger
from . import online


class _DuelingHeads:
    """True parameters of a DuelingQNetwork pair's heads (reference q_network.py:41-49) beside an engine whose output layer
    is the COMPOSED layer  W_eff = M [w_v; W_a],  b_eff = M [b_v; b_a]  with the constant M = [1 | I - 11^T/A] (A, A+1).

    Storage per network: one flat (A+1, F+1) fp32 tensor, row 0 = [w_v | b_v], rows 1.. = [W_a[j] | b_a[j]]; the module's
    `value.0.*` / `advantage.0.*` parameters are (strided) views of it, Adam moments mirror it.  After every optimizer step
    of the engine: gather the output layer's gradient (A, F+1) from the engine's gradient group, map it back with
    M^T (one TN product on porl_gemm_f32), torch-exact Adam on the heads (porl_adam_ema, the trainer's step counter and
    hyper-parameters), compose (one NN product) and write the composed layer into the engine's parameter image.  The
    engine's own Adam also steps the composed layer — overwritten right away, its moments are never used.  All arithmetic
    is HIP kernels; torch only copies between strided views."""

    def __init__(self, trainer, q_network, target_network):
        eng = trainer._engine
        self.trainer, self.eng = trainer, eng
        A, F = eng.cfg.n_actions, 64
        self.A, self.F = A, F
        dev = eng.device
        n = ((A + 1) * (F + 1) + 3) // 4 * 4
        z = lambda: torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat, self.flat_tgt, self.grad, self.m, self.v = z(), z(), z(), z(), z()
        M = torch.zeros(A, A + 1, dtype=torch.float32)
        M[:, 0] = 1.0
        M[:, 1:] = torch.eye(A) - 1.0 / A
        self.M = M.to(dev)
        self.g_ext = torch.zeros(A, F + 1, dtype=torch.float32, device=dev)
        self.w_ext = torch.zeros(A, F + 1, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for mod, flat in ((q_network, self.flat), (target_network, self.flat_tgt)):
                hd = flat[:(A + 1) * (F + 1)].view(A + 1, F + 1)
                for p, v in ((mod.value[0].weight, hd[0:1, :F]), (mod.value[0].bias, hd[0, F:F + 1]),
                             (mod.advantage[0].weight, hd[1:, :F]), (mod.advantage[0].bias, hd[1:, F])):
                    v.copy_(p)
                    p.data = v
        self.compose(0)
        self.flat_tgt_sync = False

    def _hd(self, flat):
        return flat[:(self.A + 1) * (self.F + 1)].view(self.A + 1, self.F + 1)

    def compose(self, which):
        """Write the composed output layer of the online (0) / target (1) network into the engine's parameter image."""
        A, F, eng = self.A, self.F, self.eng
        hd = self._hd(self.flat if which == 0 else self.flat_tgt)
        E.gemm_f32(1, self.M, hd, A, F + 1, A + 1, A + 1, F + 1, self.w_ext, F + 1)          # (A, A+1) x (A+1, F+1)
        views = eng.views(eng.params if which == 0 else eng.params_tgt)
        with torch.no_grad():
            views[-2].copy_(self.w_ext[:, :F])
            views[-1].copy_(self.w_ext[:, F])

    def after_step(self, hp):
        A, F, eng = self.A, self.F, self.eng
        gv = eng.views(eng.grads)
        with torch.no_grad():
            self.g_ext[:, :F].copy_(gv[-2])
            self.g_ext[:, F].copy_(gv[-1])
        # d(heads) = M^T d(composed layer): "TN" product, contraction over the A composed rows
        E.gemm_f32(2, self.M, self.g_ext, A + 1, F + 1, A, A + 1, F + 1, self._hd(self.grad), F + 1)
        g = self.trainer.optimizer.param_groups[0]
        E.adam_ema(self.flat, self.grad, self.m, self.v, None, hp.lr, hp.step, g["betas"][0], g["betas"][1], g["eps"], 0.0)
        self.compose(0)

    def after_sync(self):
        with torch.no_grad():
            self.flat_tgt.copy_(self.flat)
        # (the engine copied the online image, composed layer included, into the target image)


class _FlatAdam:
    """torch.optim.Adam-format state over the engine's flat group (see agent/_iql.py:ArenaAdam)."""

    def __init__(self, engine, params, lr):
        self._eng, self._params, self.step_count = engine, params, 0
        self.param_groups = [dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, params=params)]

    def zero_grad(self, set_to_none=True):
        pass

    def hyper(self, gamma, alpha, inv_batch):
        """QnetHyper of the next Adam step (step_count + 1); nothing advances.  After the native call(s) made with it
        the caller sets `step_count = hp.step` — a call that was refused leaves the step number with the moments."""
        g = self.param_groups[0]
        return self._eng.hyper(gamma, alpha, inv_batch, self.step_count + 1, g["lr"], g["betas"], g["eps"])

    _dueling = None      # _DuelingHeads of a DuelingQNetwork trainer: the heads' moments live beside the engine's

    def _moments(self):
        ms, vs = self._eng.views(self._eng.adam_m), self._eng.views(self._eng.adam_v)
        if self._dueling is not None:
            # q_network.parameters() order: value.w, value.b, advantage.w, advantage.b, then the hidden layers (the engine's
            # last two tensors are the composed output layer, which is not a parameter)
            d = self._dueling
            hm, hv = d._hd(d.m), d._hd(d.v)
            pick = lambda h: [h[0:1, :d.F], h[0, d.F:d.F + 1], h[1:, :d.F], h[1:, d.F]]
            return pick(hm) + ms[:-2], pick(hv) + vs[:-2]
        return ms, vs

    def state_dict(self):
        ms, vs = self._moments()
        state = {i: dict(step=torch.tensor(float(self.step_count)), exp_avg=m.clone(), exp_avg_sq=v.clone())
                 for i, (m, v) in enumerate(zip(ms, vs))} if self.step_count else {}
        g = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        g["params"] = list(range(len(self._params)))
        return dict(state=state, param_groups=[g])


def read_losses(trainer, penalty=False):
    """[loss, td_loss, cql_penalty] of the step just launched on trainer._engine: the device view with async_losses, else
    one read-back that returns the loss and keeps last_td_loss (and, with `penalty`, last_cql_penalty)."""
    stats = trainer._engine.stats[:3]
    if trainer.async_losses:
        return stats
    loss, trainer.last_td_loss, pen = stats.tolist()
    if penalty:
        trainer.last_cql_penalty = pen
    return loss


def checked_loss(loss, actions, n_actions):
    """`loss` (a float) — or the reference's IndexError: its `gather` raises on a minibatch with an action outside
    0..A-1 (qr_dqn_trainer.py:147, c51_trainer.py:155); the loss-head kernels make no access through a bad index, the row
    gets a NaN loss term and no gradient.  `actions`: callable giving the minibatch's actions, called only on a NaN."""
    if loss != loss:
        a = actions()
        if not bool(((a >= 0) & (a < n_actions)).all()):
            raise IndexError("action index out of range in the minibatch (valid: 0..%d)" % (n_actions - 1))
    return loss


def learn_minibatch(eng, opt, gamma, alpha, batch, variant):
    """One step of `eng` on an explicit minibatch (device tensors): the step kernel on rows 0..B-1 of the minibatch
    itself (learn_indexed, so every QnetVariant applies).  Returns the engine's statistics."""
    states, actions, rewards, next_states, dones = batch
    states, next_states = eng._states(states).contiguous(), eng._states(next_states, "next_states").contiguous()
    B = states.shape[0]
    hp = opt.hyper(gamma, alpha, 1.0 / B)
    idx = torch.arange(B, dtype=torch.int64, device=eng.device)
    eng.learn_indexed(hp, states, actions.long().contiguous(), rewards.float().contiguous(), next_states,
                      dones.float().contiguous(), idx, variant=variant)
    opt.step_count = hp.step
    return eng.stats


class CQLTrainer:
    def __init__(self, state_size, action_size, gamma, epsilon=1.0, epsilon_min=0.05, epsilon_decay=0.99,
                 update_target_freq=10, device=torch.device("cpu"), network=QNetwork, log_dir="logs",
                 num_epochs=1000, threshold=0.1, alpha=1, learning_rate=0.0005, replay_buffer=None,
                 batch_size=64, max_batch=4096, transition_learning_step=10000):
        self.state_size, self.action_size = state_size, action_size
        self.device = torch.device(device)
        self.gamma, self.epsilon, self.epsilon_min, self.epsilon_decay = gamma, epsilon, epsilon_min, epsilon_decay
        self.learning_rate, self.update_target_freq = learning_rate, update_target_freq
        self.num_epochs, self.threshold, self.alpha = num_epochs, threshold, alpha
        self.training_learning_step = transition_learning_step       # train_online's learn threshold (dqn_trainer.py:62)
        # same construction order / RNG consumption as dqn_trainer.py:66-70; `network` is any callable (state_size,
        # action_size) -> QNetwork, e.g. `lambda s, a: QNetwork(s, a, [256, 256])` for other hidden sizes
        self.q_network = network(state_size, action_size)
        self.target_network = network(state_size, action_size)
        dueling = isinstance(self.q_network, DuelingQNetwork) and isinstance(self.target_network, DuelingQNetwork)
        if not dueling and (not isinstance(self.q_network, QNetwork) or not isinstance(self.target_network, QNetwork)):
            raise NotImplementedError("QNetwork (a plain Linear/ReLU chain) and DuelingQNetwork are on the accelerated path")
        hidden = self.q_network._spec[2]
        self._engine = QnetEngine(state_size, action_size, hidden, max(max_batch, batch_size), self.device)
        for which, mod in enumerate((self.q_network, self.target_network)):
            # dueling: `model` holds the hidden layers only; the engine's output layer is the composed layer
            self._engine.adopt(mod, which, list(mod.model.parameters()) if dueling else None)
        if not dueling:
            with torch.no_grad():
                self._engine.params_tgt.copy_(self._engine.params)   # target.load_state_dict(q.state_dict())
        self._dueling = None
        if dueling:
            self._engine._ensure_bound()
            self._dueling = _DuelingHeads(self, self.q_network, self.target_network)
            # target.load_state_dict(q.state_dict()) (dqn_trainer.py:68): hidden layers, composed layer and heads
            self._engine.params_tgt.copy_(self._engine.params)
            self._dueling.after_sync()
            self._engine.post_step, self._engine.post_sync = self._dueling.after_step, self._dueling.after_sync
            for mod, which in ((self.q_network, 0), (self.target_network, 1)):
                mod.register_load_state_dict_post_hook(lambda module, incompatible, w=which: self._dueling.compose(w))
        self.target_network.eval()
        self.optimizer = _FlatAdam(self._engine, list(self.q_network.parameters()), learning_rate)
        self.optimizer._dueling = self._dueling
        self.replay_buffer = replay_buffer if replay_buffer is not None else ReplayBuffer(100000, (state_size,), self.device)
        self.batch_size = batch_size
        self.logger = Logger(log_dir=log_dir)
        self.logger.log_hyperparameters(dict(learning_rate=learning_rate, gamma=gamma, batch_size=batch_size,
                                             epsilon_decay=epsilon_decay, update_target_freq=update_target_freq))
        self.training_step = 0
        self._exchange = GradExchange()
        self.async_losses = False

    # -- hot path ---------------------------------------------------------------------------------
    def learn_on(self, states, actions, rewards, next_states, dones):
        """cql_trainer.py:94-124 on an explicit minibatch (device tensors)."""
        eng, ex = self._engine, self._exchange
        B = eng.load_batch(states, actions, rewards, next_states, dones)
        hp = self.optimizer.hyper(self.gamma, float(self.alpha), 1.0 / (B * ex.world_size))
        if not ex.active:
            eng.learn(hp)
        else:
            eng.cql_backward(hp)
            ex.allreduce_sum_(eng.grads)
            ex.allreduce_sum_(eng.stats[:3])
            eng.apply(hp)
        self.optimizer.step_count = hp.step
        return read_losses(self, penalty=True)

    def learn(self):
        return self.learn_on(*self.replay_buffer.sample(self.batch_size))

    _rows_for = learn_on          # the learn_on that _learn_rows reproduces (a subclass overriding learn_on opts out)

    def _learn_rows(self, idx):
        """learn_on on rows `idx` (device int64) of the replay mirror, gathered inside the step kernel."""
        eng, m = self._engine, self.replay_buffer._mirror
        hp = self.optimizer.hyper(self.gamma, float(self.alpha), 1.0 / idx.numel())
        eng.learn_indexed(hp, m["states"], m["actions"], m["rewards"], m["next_states"], m["dones"], idx,
                          variant=self._rows_variant())
        self.optimizer.step_count = hp.step

    def _rows_variant(self):
        return None

    def learn_device_sampled(self, seed=0):
        """Extension (not in the reference): `learn()` with the B distinct indices drawn on the device (keyed
        permutation) instead of numpy's O(N) host permutation — no host work, no host->device copies."""
        rb = self.replay_buffer
        if self.batch_size > rb.size:
            raise ValueError("Cannot take a larger sample than population when 'replace=False'")
        rb._sync_mirror()
        self._draws = getattr(self, "_draws", 0)
        draw = self._draws
        self._draws += 1
        eng, ex = self._engine, self._exchange
        if ex.active or not eng.fused:
            idx = E.sample_indices(rb.size, self.batch_size, seed, draw, device=self.device)
            return self.learn_on(*rb.gather_device(idx))
        # one-launch path: the step kernel draws the rows itself (or gathers rows idx of the device mirror)
        m = rb._mirror
        hp = self.optimizer.hyper(self.gamma, float(self.alpha), 1.0 / self.batch_size)
        if eng.can_sample:
            eng.learn_sampled(hp, m["states"], m["actions"], m["rewards"], m["next_states"], m["dones"], rb.size,
                              self.batch_size, seed, draw)
        else:
            idx = E.sample_indices(rb.size, self.batch_size, seed, draw, device=self.device)
            eng.learn_indexed(hp, m["states"], m["actions"], m["rewards"], m["next_states"], m["dones"], idx)
        self.optimizer.step_count = hp.step
        return read_losses(self, penalty=True)

    def compute_cql_penalty(self, states, actions):
        return self._engine.penalty(states, actions)

    def sync_target(self):
        self._engine.sync_target()

    def train_offline(self, policy=None, num_iterations: int = 10000):
        return online.run_offline(self, policy, num_iterations)

    def train_online(self, env, policy=None, num_episodes: int = 1000, max_steps: int = 1000):
        """dqn_trainer.py:119-180 (train/online.py): learns once len(replay_buffer) >= training_learning_step; greedy
        actions, pushes and learn steps take the one-launch forms when the network and buffer allow."""
        fast = None
        cls = type(self)
        if online.fast_ok(self) and cls._act_for is cls.select_action and cls._greedy_for is cls.get_action:
            rows = cls.learn is CQLTrainer.learn and cls._rows_for is cls.learn_on and not self._exchange.active
            fast = online._Fast(self, learn_rows=self._learn_rows if rows else None)
        return online.run(self, env, policy, num_episodes, max_steps, self.training_learning_step, self.replay_buffer,
                          self.replay_buffer.push, fast)

    def train_vectorized(self, sim, n_steps, **kw):
        """act -> step -> learn with the N robots of a DiscreteLidarNavSim and no host synchronisation inside the loop
        (train/vector_online.py).  PER and BCQ trainers raise NotImplementedError: they run through train_online(Env(...))."""
        from .vector_online import train_vectorized
        return train_vectorized(self, sim, n_steps, **kw)

    def train_offline_device(self, replay, n_iters, **kw):
        """`n_iters` learn steps on a DeviceReplay with the minibatches drawn on the device and nothing read back inside the
        loop (train/vector_offline.py).  PER trainers raise NotImplementedError."""
        from .vector_offline import train_offline_device
        return train_offline_device(self, replay, n_iters, **kw)

    # -- acting -----------------------------------------------------------------------------------
    def get_action(self, state: np.ndarray) -> int:
        x = torch.as_tensor(np.asarray(state), dtype=torch.float32, device=self.device).unsqueeze(0)
        return int(self.q_network(x).argmax(dim=1).item())

    def select_action(self, state: np.ndarray) -> int:
        if np.random.rand() < self.epsilon:
            return int(np.random.randint(self.action_size))
        return self.get_action(state)

    _act_for, _greedy_for = select_action, get_action      # the action rule porl_qnet_act reproduces in train_online

    def greedy_action(self, state: np.ndarray) -> int:
        """get_action(state) in one launch (porl_qnet_act on the state carried in the kernel's arguments)."""
        eng = self._engine
        if not eng.act_ok or eng.cfg.state_dim > eng.ACT_MAX_INLINE:
            return self.get_action(state)
        if getattr(self, "_act_rec", None) is None:
            self._act_rec = torch.zeros(16, dtype=torch.int32).pin_memory()
        eng.act(self._act_rec, inline=np.asarray(state, dtype=np.float32).reshape(-1))
        torch.cuda.current_stream(eng.device).synchronize()
        return int(self._act_rec[0])
