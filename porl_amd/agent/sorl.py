"""SORL agent — drop-in for /root/reference/agent/sorl.py:20-152 on one MI355X, with or without the costmap
encoder as `backbone` (sorl_train.py:29-33: `FasterNet(3, args.feature_dim)`, porl_amd/agent/fasternet.py).

Same constructor and attribute names (`v_net`, `policy`, `v_tgt`, `v_optimizer`, `policy_optimizer`,
`lr_schedule`), `update`, `vf_update`, `policy_update`, `select_action`.  Value step == POR's; the policy step is
advantage-weighted behaviour cloning of the dataset actions with a tanh-bounded mean and
weight = min(exp(alpha * adv), 100) — alpha MULTIPLIES here (sorl.py:104), unlike POR.

`policy_update` (sorl.py:154-176), the policy phase of the two-phase script sorl_train_v0.py:57-103, is broken upstream:
it reads `target_v` (sorl.py:163) without assigning it.  Here it behaves as evidently intended: the two missing lines are
taken from `update` / `vf_update` of the same file (sorl.py:85-89), `next_v = v_tgt(s')` without gradient and
`target_v = r + (1 - d) * discount * next_v`; everything else is the method as written.  It runs as a step of its own
on the device (five forward-only nets per layer in one launch, one head kernel for target, advantage and weight, the
policy's backward and Adam) and leaves the value nets, the target nets and the value optimizer untouched.
`vf_update_from_replay` / `policy_update_from_replay` are the two phases on rows drawn on the device; like
`update_from_replay` they work with a backbone (rows encoded in place in the store).  `update_from_replay` also takes
`indices=` to name the rows instead of drawing them.
"""
from __future__ import annotations

import copy

import torch

from ._iql import ArenaAdam, CosineSchedule, IqlAgentBase, evaluate_store  # noqa: F401
from .policy import BoundedGaussianPolicy
from .value_functions import TwinV

EXP_ADV_MAX = 100.


class SORL(IqlAgentBase):
    def __init__(agent, args, max_steps, tau, alpha, device=torch.device('cpu'), backbone=None,
                 value_lr=1e-4, policy_lr=1e-4, discount=0.99, beta=0.005):
        super().__init__()
        agent.device = torch.device(device)
        agent.backbone = backbone
        # with a backbone the heads see its features (sorl.py:46-56); it joins no optimizer (sorl.py:58-64)
        in_dim = args.state_size if backbone is None else args.feature_dim
        if backbone is not None:
            agent.backbone = backbone.to(agent.device)
        # SORL builds the value net BEFORE the policy (sorl.py:37-45)
        agent.v_net = TwinV(in_dim, layer_norm=args.layer_norm,
                            hidden_dim=args.hidden_dim, n_hidden=args.n_hidden)
        agent.policy = BoundedGaussianPolicy(in_dim, args.action_size,
                                             hidden_dim=args.hidden_dim, n_hidden=args.n_hidden)
        agent.v_tgt = copy.deepcopy(agent.v_net).requires_grad_(False)
        agent._setup_engine(agent.v_net, agent.v_tgt, agent.policy,
                            obs_dim=in_dim, pol_out_dim=args.action_size, hidden_dim=args.hidden_dim,
                            n_hidden=args.n_hidden, layer_norm=args.layer_norm, pol_tanh=True, weight_mode=1,
                            device=agent.device, max_batch=int(getattr(args, "max_batch", 0) or
                                                               getattr(args, "batch_size", 0) or 1024))
        agent.v_optimizer = ArenaAdam(agent, 0, list(agent.v_net.named_parameters()), value_lr)
        agent.policy_optimizer = ArenaAdam(agent, 1, list(agent.policy.named_parameters()), policy_lr)
        agent.lr_schedule = CosineSchedule(agent.policy_optimizer, max_steps)
        agent.tau = tau
        agent.alpha = alpha
        agent.discount = discount
        agent.beta = beta

    def select_action(agent, observations):
        """Mean action as a numpy array (reference sorl.py:71-76)."""
        agent.flush()
        if agent.backbone is not None:
            observations = agent.backbone(observations)
        return agent.policy.mean_numpy(observations)

    def update(agent, observations, actions, rewards, next_observations, terminals):
        """Joint value + policy step (reference sorl.py:78-128) -> (v_loss, g_loss).  With a backbone both
        observation batches are encoded first, s then s' (sorl.py:81-83); the encoder is forward-only because
        nothing ever consumes its gradients."""
        if agent.backbone is not None:
            observations = agent.backbone(observations)
            next_observations = agent.backbone(next_observations)
        return agent._full_update(observations, next_observations, rewards, terminals, actions,
                                  agent.v_optimizer, agent.policy_optimizer, agent.lr_schedule)

    def evaluate(agent, observations, actions, rewards, next_observations, terminals):
        """Extension (not in the reference): (v_loss, g_loss) of the parameters as they stand on this batch, WITHOUT a
        step — the loss of `update`'s value phase, and the policy's weighted NLL on the actions with the weight
        min(exp(alpha * adv), 100) taken from the current online twin.  Every parameter, the target nets, both Adam
        moments and step counts and the cosine schedule stay bit for bit; an outstanding pipelined phase is flushed
        first; gradient buffers, workspace and the statistics buffer are scratch.  With `async_losses` the statistics
        view is returned, as by the update calls.  Under a data-parallel exchange the losses are this rank's own.  With
        a backbone: NotImplementedError.  `evaluate_from_replay` / `evaluate_store` score rows of a store."""
        agent._evaluate(observations, next_observations, rewards, terminals, actions)
        return agent._losses()

    def vf_update(agent, observations, actions, rewards, next_observations, terminals):
        """Value step only (reference sorl.py:130-152) -> v_loss."""
        if agent.backbone is not None:
            observations = agent.backbone(observations)
            next_observations = agent.backbone(next_observations)
        agent._value_update(observations, next_observations, rewards, terminals, agent.v_optimizer)
        if agent.async_losses:
            return agent._engine.stats[:1]
        return float(agent._engine.stats[0])

    def policy_update(agent, observations, actions, rewards, next_observations, terminals):
        """Policy step only, value nets frozen (reference sorl.py:154-176, with the TD target of sorl.py:85-89 that the
        reference method reads but never assigns) -> g_loss."""
        if agent.backbone is not None:
            observations = agent.backbone(observations)
            next_observations = agent.backbone(next_observations)
        agent._policy_update(observations, next_observations, rewards, terminals, actions,
                             agent.policy_optimizer, agent.lr_schedule)
        return agent._policy_loss()

    def vf_update_from_replay(agent, replay, batch_size):
        """Extension (not in the reference): `vf_update` on rows drawn on the device from a PackedReplay; with a backbone
        the rows are encoded where they lie in the store (see `update_from_replay`)."""
        idx, feats = agent._replay_rows(replay, batch_size, None)
        agent._value_update(None, None, None, None, agent.v_optimizer, replay=replay, batch=batch_size, idx=idx, feats=feats)
        if agent.async_losses:
            return agent._engine.stats[:1]
        return float(agent._engine.stats[0])

    def policy_update_from_replay(agent, replay, batch_size):
        """Extension (not in the reference): `policy_update` on rows drawn on the device from a PackedReplay; with a
        backbone the rows are encoded where they lie in the store (see `update_from_replay`)."""
        idx, feats = agent._replay_rows(replay, batch_size, None)
        agent._policy_update(None, None, None, None, None, agent.policy_optimizer, agent.lr_schedule,
                             replay=replay, batch=batch_size, idx=idx, feats=feats)
        return agent._policy_loss()

    def update_from_replay(agent, replay, batch_size, indices=None):
        """Extension (not in the reference): `update` on `batch_size` rows of a PackedReplay — drawn on the device, or the
        local row numbers in `indices` (int64 device tensor; the replay's draw counter then stays put).  Same arithmetic
        as `update` on those rows, bit for bit.  With a backbone, s then s' are encoded where they lie in the store
        (`FasterNet.forward_rows`), which is only read.  Raises ValueError when the replay's state width is not the
        agent's."""
        idx, feats = agent._replay_rows(replay, batch_size, indices)
        return agent._full_update(None, None, None, None, None, agent.v_optimizer, agent.policy_optimizer,
                                  agent.lr_schedule, replay=replay, batch=batch_size, idx=idx, feats=feats)
