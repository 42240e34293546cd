"""Discrete BCQ trainer — drop-in for /root/reference/src/porl/train/bcq_trainer.py:18-82 on one MI355X: a `DQNTrainer`
plus a behaviour-policy model and its optimizer (Adam, lr 5e-4), `num_epochs`, `threshold`.  The two update rules live
in porl_amd/policy/bcq.py like upstream (`bcq_learn`, `bcq_behavior_pretrain`); both run on the one-launch Q-network
step kernel (csrc/qnet_fused.hpp) — the behaviour policy is just another small MLP with its own flat parameter group."""
from __future__ import annotations

import torch

from ..net.behavior_policy import BehaviorPolicy
from ..net.q_network import QNetwork
from ..engine import QnetEngine
from .cql_trainer import _FlatAdam
from .dqn_trainer import DQNTrainer


class BCQTrainer(DQNTrainer):
    def __init__(self, state_size, action_size, gamma, epsilon=1.0, epsilon_min=0.05, epsilon_decay=0.99,
                 update_target_freq=10, device=torch.device("cpu"), network=QNetwork, behavior_policy=BehaviorPolicy,
                 log_dir="logs", num_epochs=1000, threshold=0.1, **kw):
        super().__init__(state_size, action_size, gamma, epsilon, epsilon_min, epsilon_decay, update_target_freq, device,
                         log_dir=log_dir, network=network, **kw)
        self.num_epochs, self.threshold = num_epochs, threshold
        # bcq_trainer.py:59-62 (constructed after the Q-networks: same RNG consumption order)
        self.behavior_policy = behavior_policy(state_size, action_size)
        hidden = self.behavior_policy._spec[2]
        eng = QnetEngine(state_size, action_size, hidden, self._engine.cfg.max_batch, self.device)
        eng.adopt(self.behavior_policy)
        self._behavior_engine = eng
        self.behavior_optimizer = _FlatAdam(eng, list(self.behavior_policy.parameters()), 0.0005)

    def train(self, env, policy, num_episodes=1000, max_steps=1000, **kwargs):
        """bcq_trainer.py:64-82: optional dataset collection and behaviour pre-training, then the training loop.
        Upstream ends in `super().train(env, policy, num_episodes, max_steps)`, a method DQNTrainer does not have; the
        argument list is train_online's, whose loop calls `policy()` without arguments.  With `policy=bcq_learn` (the
        function object, as scripts/train_bcq.py passes it) this is read as the online loop with bcq_learn bound to
        this trainer.  Any other policy keeps the offline loop: `train_offline(policy, num_episodes)`."""
        from ..policy.bcq import bcq_learn
        if "dataset" in kwargs:
            kwargs["dataset"](env, self)
        if "pretrain" in kwargs:
            kwargs["pretrain"](self)
        if policy is bcq_learn:
            return self.train_online(env, bcq_learn, num_episodes, max_steps)
        return self.train_offline(policy=policy, num_iterations=num_episodes)

    def act_rows(self, states, epsilon, seed, t, env_offset=0, constrained=True, **scratch):
        """Epsilon-greedy actions (n,) int64 on the device for n rows of states.  `constrained=True` (an extension over the
        reference's trainer): the rule bcq_learn's target assumes — the best action among those the behaviour policy allows
        at `self.threshold` (QnetEngine.act_rows_bcq; scratch q, logits, mask, out).  `constrained=False`: the plain arg-max
        the reference's trainer acts with (QnetEngine.act_rows; scratch q, out).  Exploration is unconstrained either way."""
        if not constrained:
            return self._engine.act_rows(states, epsilon, seed, t, env_offset=env_offset, **scratch)
        return self._engine.act_rows_bcq(self._behavior_engine, states, self.threshold, epsilon, seed, t, env_offset=env_offset,
                                         **scratch)

    def train_offline_device(self, replay, n_iters, **kw):
        """Behaviour pre-training and `n_iters` BCQ steps on a DeviceReplay, nothing read back inside the loops
        (train/vector_offline.py)."""
        from .vector_offline import train_offline_device
        return train_offline_device(self, replay, n_iters, **kw)

    def train_online(self, env, policy=None, num_episodes: int = 1000, max_steps: int = 1000):
        """dqn_trainer.py:119-180.  `policy=bcq_learn` (the function of porl_amd.policy.bcq): the loop with the BCQ rule
        bound to this trainer — greedy act and record on their one-launch forms, each learn step numpy's index draw into
        bcq_learn_rows (one native call: mask kernel, step kernel, reduction + Adam), the loss deferred; off the fast
        path the reference loop with `lambda: bcq_learn(self)`.  Any other policy: DQNTrainer.train_online."""
        from . import online
        from ..policy import bcq
        if policy is not bcq.bcq_learn:
            return super().train_online(env, policy, num_episodes, max_steps)
        cls = type(self)
        fast = None
        if online.fast_ok(self) and cls._act_for is cls.select_action and cls._greedy_for is cls.get_action and \
                not self._exchange.active:
            fast = online._FastBCQ(self)
        return online.run(self, env, None if fast is not None else (lambda: bcq.bcq_learn(self)), num_episodes, max_steps,
                          self.training_learning_step, self.replay_buffer, self.replay_buffer.push, fast)
