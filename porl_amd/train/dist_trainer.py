"""Shared host logic of the distributional trainers (QR-DQN, C51) on the Q-network engine's general path:

    sample (reference index stream) -> load -> online forward on s (activations kept) -> forward passes on s' ->
    loss head kernel (csrc/dist_losses.hpp: dL/d(output) + per-row loss) -> backward -> Adam

Every arithmetic step is a HIP kernel behind the C ABI.  The calls on the engine's handle (porl_qnet_forward_loaded /
porl_qnet_backward / porl_qnet_apply / porl_qnet_dist_learn) are methods of engine.QnetEngine, which also checks the
replay arrays (engine.replay_args); only the stateless loss heads (porl_qr_loss / porl_c51_loss / porl_reduce_mean) are
called from the trainers.  The Adam step number advances after the native call that used it (cql_trainer._FlatAdam.hyper),
and the reference's IndexError on a bad action is cql_trainer.checked_loss.  The output layer is wider than the one-launch step kernel's
128 columns (actions x quantiles), so these trainers use the grouped-GEMM path like any wide Q-network.

`learn_indexed(idx)` is the same step on rows `idx` of the replay mirror from ONE native call (porl_qnet_dist_learn:
gather, the forwards grouped per layer, loss head on the padded rows, mean loss into the engine's statistics, backward,
Adam) — bit-equal parameters, moments and loss, no copies between the stages; `train_online` learns through it.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native as N
from ..buffer.replay_buffer import ReplayBuffer
from ..parallel import GradExchange
from ..utils.logger import Logger
from ..engine import QnetEngine
from . import online
from .cql_trainer import _FlatAdam, checked_loss


class DistTrainerBase:
    """Common attributes of the reference's DQNTrainer subclasses: q_network, target_network, optimizer,
    replay_buffer, batch_size, gamma, epsilon*, update_target_freq, device, logger."""

    def _setup(self, q_network, target_network, state_size, action_size, gamma, epsilon, epsilon_min, epsilon_decay,
               update_target_freq, device, learning_rate, log_dir, batch_size, max_batch, replay_buffer,
               transition_learning_step=10000):
        self.state_size, self.action_size = state_size, action_size
        self.device = torch.device(device)
        self.gamma, self.epsilon, self.epsilon_min, self.epsilon_decay = gamma, epsilon, epsilon_min, epsilon_decay
        self.learning_rate, self.update_target_freq = learning_rate, update_target_freq
        self.q_network, self.target_network = q_network, target_network
        s, n_out, hidden = q_network._spec
        self._engine = eng = QnetEngine(s, n_out, hidden, max(max_batch, batch_size), self.device)
        eng.adopt(q_network, 0)
        eng.adopt(target_network, 1)
        with torch.no_grad():
            eng.params_tgt.copy_(eng.params)                           # target.load_state_dict(q.state_dict())
        target_network.eval()
        self.optimizer = _FlatAdam(eng, list(q_network.parameters()), learning_rate)
        self.replay_buffer = replay_buffer if replay_buffer is not None else ReplayBuffer(100000, (state_size,), self.device)
        self.batch_size = batch_size
        self.training_learning_step = transition_learning_step     # train_online's learn threshold (dqn_trainer.py:62)
        self.logger = Logger(log_dir=log_dir)
        self.async_losses = False
        self._exchange = GradExchange()         # train_online keeps the plain loop while a gradient exchange is active
        mb = eng.cfg.max_batch
        self._out = [torch.empty(mb, n_out, dtype=torch.float32, device=self.device) for _ in range(3)]
        self._dout = torch.empty(mb, n_out, dtype=torch.float32, device=self.device)
        self._row_loss = torch.empty(mb, dtype=torch.float32, device=self.device)
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)

    # -- engine pieces ----------------------------------------------------------------------------------
    def _backward_and_step(self, dout, B):
        eng = self._engine
        eng.backward(dout)
        hp = self.optimizer.hyper(self.gamma, 0.0, 1.0 / B)
        eng.apply(hp)
        self.optimizer.step_count = hp.step
        N.check(N.lib().porl_reduce_mean(N.ptr(self._row_loss), B, N.ptr(self._loss), N.current_stream_ptr(eng.device)),
                "porl_reduce_mean")
        if self.async_losses:
            return self._loss
        return checked_loss(float(self._loss), lambda: self._actions, self.action_size)

    def _load(self, batch):
        states, actions, rewards, next_states, dones = batch
        B = self._engine.load_batch(states, actions, rewards, next_states, dones)
        self._actions = actions = actions.long().contiguous()
        return B, actions, rewards.float().contiguous(), dones.float().contiguous()

    def learn(self):
        return self.learn_on(*self.replay_buffer.sample(self.batch_size))

    # -- the same step on rows of the replay mirror, one native call -------------------------------------------------
    _rows_for = None                   # the subclass's learn_on that _dist_head describes (overriding learn_on opts out)

    def _dist_head(self):
        """N.DistHead of this trainer's loss (kind, actions, quantiles / atoms, kappa, v_min, v_max, support)."""
        raise NotImplementedError

    def _learn_rows(self, idx):
        """Launch learn_on on rows `idx` (device int64) of the replay mirror; the mean loss lands in eng.stats[0]."""
        eng, m = self._engine, self.replay_buffer._mirror
        hp = self.optimizer.hyper(self.gamma, 0.0, 1.0 / max(idx.numel(), 1))      # (an empty idx is the engine's to refuse)
        eng.dist_learn(hp, m["states"], m["actions"], m["rewards"], m["next_states"], m["dones"], idx, self._dist_head())
        self.optimizer.step_count = hp.step

    def learn_indexed(self, idx):
        """learn_on(*replay_buffer.sample_at(idx)) from one native call: same parameters, Adam moments and loss, bit for
        bit.  `idx`: int64 row numbers of the replay buffer (device tensor, or anything numpy converts)."""
        if self.device.type != "cuda":
            raise N.NativeError("porl_amd computes on a HIP device only (device='cuda'); there is no CPU path")
        if not torch.is_tensor(idx):
            idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(self.device)
        self.replay_buffer._sync_mirror()
        self._learn_rows(idx)
        stats = self._engine.stats
        if self.async_losses:
            return stats[:1]
        return checked_loss(float(stats[0]), lambda: self.replay_buffer._mirror["actions"][idx], self.action_size)

    def sync_target(self):
        self._engine.sync_target()

    def train_offline(self, policy=None, num_iterations: int = 10000):
        losses = []
        for step in range(num_iterations):
            losses.append(self.learn() if policy is None else policy())
            if step % self.update_target_freq == 0:
                self.sync_target()
        return losses

    def _greedy(self, q_values):
        return int(q_values.argmax(dim=1).item())

    # -- online loop (train/online.py) --------------------------------------------------------------------------------
    _online_threshold = "transition"   # dqn_trainer.py:148 (QR-DQN inherits it); C51 overrides: "batch" (c51_trainer.py:205)
    _act_for = None                    # the subclass's select_action that _act_epilogue reproduces

    def _act_epilogue(self):
        """(kind, n_sub, support) of porl_qnet_act for this network's greedy rule."""
        raise NotImplementedError

    def train_online(self, env, policy=None, num_episodes: int = 1000, max_steps: int = 1000):
        """dqn_trainer.py:119-180 / c51_trainer.py:176-225; greedy actions and pushes take the one-launch forms when the
        network fits the act kernel, and the learn step runs from one native call on the sampled rows of the mirror
        (_learn_rows; its loss is read with the next act record) unless a subclass overrides learn / learn_on or a
        gradient exchange is active — then learn() as it stands."""
        fast = None
        cls = type(self)
        if online.fast_ok(self) and cls._act_for is cls.select_action:
            kind, n_sub, support = self._act_epilogue()
            rows = cls.learn is DistTrainerBase.learn and cls._rows_for is not None and cls._rows_for is cls.learn_on \
                and not self._exchange.active
            fast = online._Fast(self, kind=kind, n_sub=n_sub, support=support, learn_rows=self._learn_rows if rows else None)
        threshold = self.batch_size if self._online_threshold == "batch" else self.training_learning_step
        return online.run(self, env, policy, num_episodes, max_steps, threshold, self.replay_buffer,
                          self.replay_buffer.push, fast)

    def train_vectorized_dist(self, sim, n_steps, **kw):
        """act -> step -> learn with the N robots of a DiscreteLidarNavSim and no host synchronisation inside the loop:
        train/vector_online.py (`train_vectorized`, the plain-Q loop, keeps turning these trainers away)."""
        from .vector_online import train_vectorized_dist
        return train_vectorized_dist(self, sim, n_steps, **kw)
