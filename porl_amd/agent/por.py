"""POR agent — drop-in for /root/reference/agent/por.py:20-112 on one MI355X.

Same constructor, attributes (`goal_policy`, `vf`, `v_target`, `v_optimizer`, `goal_policy_optimizer`,
`goal_lr_schedule`, `tau`, `alpha`, `discount`, `beta`), `state_dict()` keys and
`por_residual_update(observations, next_observations, rewards, terminals) -> (v_loss, g_loss)`.
All arithmetic of the update (and of `goal_policy(obs)`, `vf.both(obs)`) runs in hand-written gfx950 kernels
(porl_amd/csrc).  Torch tensor ops on the device remain only in off-path conveniences: `DiagGaussian.log_prob / sample`
on caller-supplied values (agent/policy.py), the stand-alone EMA on odd-sized tensors (util/util.py), and the replay
mirror's scatter of newly pushed transitions (buffer/replay_buffer.py).

Deliberate differences from the reference (SURVEY.md §8 notes 6):
  * the `pdb.set_trace()` on NLL <= 0 (por.py:104-105) becomes a one-time RuntimeWarning;
  * dead upstream code (`pretrain*`, `save/load`, and `por_qlearning_update` but for its action-policy block, which is
    agent/goal_bc.py) is not provided;
  * with `backbone=FasterNet(...)` (por.py:46-57,75-79) the encoder runs forward-only: it joins no optimizer
    upstream, so its backward only fills gradients nobody reads.

Acting (reference test.py:29 calls `agent.select_action`, which the reference's POR does not define): POR acts through a
second policy pi(a | s, g) on [s | goal_policy mean(s)].  `set_execute_policy(bc)` takes a trained
`porl_amd.agent.goal_bc.GoalConditionedBC` (por.py:178-184), `select_action(observations)` returns its mean action.

Extension: `update_from_replay(replay, batch_size, indices=None)` runs the same step on rows of a device-resident
`PackedReplay`, drawn on the device or named by `indices`, with or without a backbone; the store is only read.
"""
from __future__ import annotations

import copy

import torch

from ._iql import ArenaAdam, CosineSchedule, IqlAgentBase, evaluate_store  # noqa: F401
from .policy import GaussianPolicy
from .value_functions import TwinV

EXP_ADV_MAX = 100.


class POR(IqlAgentBase):
    def __init__(agent, args, max_steps, tau, alpha, backbone=None, device=torch.device('cpu'),
                 value_lr=1e-4, policy_lr=1e-4, discount=0.99, beta=0.005):
        super().__init__()
        agent.device = torch.device(device)
        agent.backbone = None
        # with a backbone the heads see its features but the goal policy still predicts the raw next state (por.py:46-57)
        in_dim = args.state_size if backbone is None else args.feature_dim
        if backbone is not None:
            agent.backbone = backbone.to(agent.device)
        # construction order fixes RNG consumption and state_dict order (por.py:36-45)
        agent.goal_policy = GaussianPolicy(in_dim, args.state_size,
                                           hidden_dim=args.hidden_dim, n_hidden=args.n_hidden)
        agent.vf = TwinV(in_dim, layer_norm=args.layer_norm,
                         hidden_dim=args.hidden_dim, n_hidden=args.n_hidden)
        agent.v_target = copy.deepcopy(agent.vf).requires_grad_(False)
        agent._setup_engine(agent.vf, agent.v_target, agent.goal_policy,
                            obs_dim=in_dim, pol_out_dim=args.state_size, hidden_dim=args.hidden_dim,
                            n_hidden=args.n_hidden, layer_norm=args.layer_norm, pol_tanh=False, weight_mode=0,
                            device=agent.device, max_batch=int(getattr(args, "max_batch", 0) or
                                                               getattr(args, "batch_size", 0) or 1024))
        agent.v_optimizer = ArenaAdam(agent, 0, list(agent.vf.named_parameters()), value_lr)
        agent.goal_policy_optimizer = ArenaAdam(agent, 1, list(agent.goal_policy.named_parameters()), policy_lr)
        agent.goal_lr_schedule = CosineSchedule(agent.goal_policy_optimizer, max_steps)
        agent.tau = tau
        agent.alpha = alpha
        agent.discount = discount
        agent.beta = beta
        agent.step = 0
        agent.pretrain_step = 0

    def por_residual_update(agent, observations, next_observations, rewards, terminals):
        """One POR gradient step (reference por.py:73-112): IQL value step, EMA target update, then the
        advantage-weighted goal-policy regression on s'.  Returns (v_loss, g_loss) as Python floats."""
        target = next_observations
        if agent.backbone is not None:          # por.py:75-79: s then s' are encoded; the regression target stays the raw
            observations = agent.backbone(observations)          # next state (after the encoder's in-place > 8 clamp)
            next_observations = agent.backbone(next_observations)
        return agent._full_update(observations, next_observations, rewards, terminals, target,
                                  agent.v_optimizer, agent.goal_policy_optimizer, agent.goal_lr_schedule)

    def evaluate(agent, observations, next_observations, rewards, terminals):
        """Extension (not in the reference): (v_loss, g_loss) of the parameters as they stand on this batch, WITHOUT a
        step — the loss of `por_residual_update`'s value phase, and the goal policy's weighted NLL on s' with the
        weight min(exp(adv / alpha), 100) taken from the current online twin.  Every parameter, the target nets, both
        Adam moments and step counts and the cosine schedule stay bit for bit; an outstanding pipelined phase is
        flushed first; gradient buffers, workspace and the statistics buffer are scratch.  With `async_losses` the
        statistics view is returned, as by the update calls.  Under a data-parallel exchange the losses are this rank's
        own.  With a backbone: NotImplementedError.  `evaluate_from_replay` / `evaluate_store` score rows of a store."""
        agent._evaluate(observations, next_observations, rewards, terminals, next_observations)
        return agent._losses()

    def update_from_replay(agent, replay, batch_size, indices=None):
        """Extension (not in the reference): one POR step on `batch_size` distinct rows drawn on the device
        from a `porl_amd.buffer.replay_buffer.PackedReplay` — sampling, gather and the update without any
        host-side tensor work.  Same arithmetic as `por_residual_update` on those rows, bit for bit.
        `indices` (int64 device tensor of `batch_size` local row numbers) names the rows instead of drawing them; the
        replay's draw counter then stays put.  With a backbone, s then s' are encoded where they lie in the store
        (`FasterNet.forward_rows`): the store is never modified, entries > 8 are read as 0 by the encoder and staged as 0
        in the regression target, which is what the in-place clamp of the tensor path leaves.  Raises ValueError when the
        replay's state width is not the agent's."""
        idx, feats = agent._replay_rows(replay, batch_size, indices)
        return agent._full_update(None, None, None, None, None, agent.v_optimizer, agent.goal_policy_optimizer,
                                  agent.goal_lr_schedule, replay=replay, batch=batch_size, idx=idx, feats=feats)

    def set_execute_policy(agent, bc):
        """The action policy pi(a | s, g) POR acts through: a `GoalConditionedBC` with obs_dim = goal_dim = state_size
        (trained by its own `update` / `update_from_replay(goal="next")`).  It is held OUTSIDE the module registry: it
        has its own engine, optimizer and checkpoint, and `POR.state_dict()` keeps the reference's keys."""
        from .goal_bc import GoalConditionedBC
        if not isinstance(bc, GoalConditionedBC):
            raise TypeError(f"set_execute_policy: expected a GoalConditionedBC, got {type(bc).__name__}")
        S = agent.goal_policy._spec[1]
        if agent.backbone is not None or bc.obs_dim != agent.goal_policy._spec[0] or bc.goal_dim != S:
            raise ValueError(f"set_execute_policy: the policy acts on [{bc.obs_dim} | {bc.goal_dim}] columns, a POR agent "
                             f"without a backbone supplies [{S} | {S}]")
        agent.__dict__["_execute_policy"] = bc

    def select_action(agent, observations):
        """What reference test.py:29 calls: the action policy's mean on [obs | goal_policy mean(obs)], as a numpy array.
        `observations`: (state_size,) or (B, state_size), numpy or tensor; up to 8 rows take the host-memory path of both
        policies (`GaussianPolicy.mean_numpy`)."""
        bc = agent.__dict__.get("_execute_policy")
        if bc is None:
            raise RuntimeError("select_action: no action policy is set (POR.set_execute_policy)")
        import numpy as np
        if isinstance(observations, torch.Tensor):
            observations = observations.detach().cpu().numpy()
        observations = np.asarray(observations, dtype=np.float32)
        goal = agent.goal_policy.mean_numpy(observations)
        return bc.policy.mean_numpy(np.concatenate([observations, goal], axis=-1))
