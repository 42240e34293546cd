"""Discrete BCQ update rules — drop-ins for /root/reference/src/porl/policy/bcq.py:8-86, taking the trainer as their
argument like upstream (`agent.train(env, bcq_learn, dataset=collect_dataset, pretrain=bcq_behavior_pretrain)`).

  bcq_behavior_pretrain : `num_epochs` cross-entropy steps of the behaviour policy on replay minibatches.  The step
      kernel's conservative penalty logsumexp(z) - ln A - z[a] IS the cross-entropy up to the constant ln A, so the
      step runs with the TD term switched off (`td_off`) and alpha = 1 on the behaviour network's own parameter group.
  bcq_learn             : DQN step whose bootstrap action is the target network's best action among those the
      behaviour policy allows in s' (probability > threshold): mask from `BehaviorPolicy.sample`, masked argmax
      inside the step kernel (`next_mask`).
Minibatches come from `agent.replay_buffer.sample` (numpy's index stream, like the reference).

Device-rows forms (extensions; one native call per step, csrc/bcq_mask.hpp):
  bcq_learn_rows(agent, idx)           : bcq_learn's rule on rows `idx` (device int64) of the replay mirror — the mask
      kernel reads the rows itself, the step kernel gathers them; no gather launches, no mask round trip through torch.
  bcq_learn_device_sampled(agent, seed): the rows drawn on the device (the keyed permutation of engine.sample_indices),
      inside both kernels when the Q engine can sample.
  bcq_pretrain_device_sampled(agent, seed): `num_epochs` cross-entropy steps on device-drawn rows, one readback at the end.
With a data-parallel exchange active all three gather the rows and take the paths above.
"""
from __future__ import annotations

import math

import torch

from .. import _native as N
from .. import engine as E
from ..train.cql_trainer import learn_minibatch, read_losses


def collect_dataset(env, agent, num_episodes: int = 1000) -> None:
    """Random-policy roll-outs into `agent.replay_buffer` (bcq.py:8-20); needs a gymnasium-style environment."""
    for _ in range(num_episodes):
        state, _ = env.reset()
        done = False
        while not done:
            action = env.action_space.sample()
            next_state, reward, done, truncated, _ = env.step(action)
            done = done or truncated
            agent.replay_buffer.push(state, action, reward, next_state, done)
            state = next_state


def _step(agent, eng, opt, batch, alpha, variant):
    return learn_minibatch(eng, opt, agent.gamma, alpha, batch, variant)


def bcq_behavior_pretrain(agent):
    """bcq.py:23-47 -> list of the per-epoch cross-entropy losses (the reference prints every 10th)."""
    eng = agent._behavior_engine
    ln_a = math.log(agent.action_size)
    var = N.QnetVariant(0, None, None, None, None, 1)                  # td_off: loss = penalty = CE - ln A
    losses = []
    for epoch in range(agent.num_epochs):
        stats = _step(agent, eng, agent.behavior_optimizer, agent.replay_buffer.sample(agent.batch_size), 1.0, var)
        losses.append(stats[2] + ln_a if agent.async_losses else float(stats[2]) + ln_a)
    return losses


def bcq_learn(agent) -> float:
    """bcq.py:50-86 -> loss (float, or the device statistics view with agent.async_losses)."""
    batch = agent.replay_buffer.sample(agent.batch_size)
    mask = agent.behavior_policy.sample(batch[3], agent.threshold)      # (B, A) over next_states
    var = N.QnetVariant(0, None, None, None, mask.data_ptr(), 0)
    _step(agent, agent._engine, agent.optimizer, batch, 0.0, var)
    return read_losses(agent)


# -- device-rows forms ----------------------------------------------------------------------------------------------------
def _learn_gathered(agent, idx):
    """Today's pieces on the gathered rows (data-parallel exchange active: the step must not be fused into one call)."""
    batch = agent.replay_buffer.gather_device(idx)
    mask = agent.behavior_policy.sample(batch[3], agent.threshold)
    var = N.QnetVariant(0, None, None, None, mask.data_ptr(), 0)
    return _step(agent, agent._engine, agent.optimizer, batch, 0.0, var)


def _launch_rows(agent, idx):
    rb = agent.replay_buffer
    if agent._exchange.active:
        return _learn_gathered(agent, idx)
    eng, m = agent._engine, rb._mirror
    hp = agent.optimizer.hyper(agent.gamma, 0.0, 1.0 / idx.numel())
    eng.bcq_learn_indexed(agent._behavior_engine, hp, m["states"], m["actions"], m["rewards"], m["next_states"], m["dones"],
                          idx, agent.threshold)
    agent.optimizer.step_count = hp.step
    return eng.stats


def bcq_learn_rows(agent, idx):
    """bcq_learn on rows `idx` (device int64) of the replay mirror -> loss (float, or the device statistics view with
    agent.async_losses)."""
    agent.replay_buffer._sync_mirror()
    _launch_rows(agent, idx)
    return read_losses(agent)


def _next_draw(agent, batch):
    rb = agent.replay_buffer
    if batch > rb.size:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    rb._sync_mirror()
    agent._draws = getattr(agent, "_draws", 0)
    agent._draws += 1
    return agent._draws - 1


def bcq_learn_device_sampled(agent, seed=0):
    """bcq_learn with the B distinct rows drawn on the device (draw counter shared with learn_device_sampled)."""
    rb, eng, B = agent.replay_buffer, agent._engine, agent.batch_size
    draw = _next_draw(agent, B)
    if agent._exchange.active or not eng.can_sample:
        _launch_rows(agent, E.sample_indices(rb.size, B, seed, draw, device=agent.device))
        return read_losses(agent)
    m = rb._mirror
    hp = agent.optimizer.hyper(agent.gamma, 0.0, 1.0 / B)
    eng.bcq_learn_sampled(agent._behavior_engine, hp, m["states"], m["actions"], m["rewards"], m["next_states"], m["dones"],
                          rb.size, B, seed, draw, agent.threshold)
    agent.optimizer.step_count = hp.step
    return read_losses(agent)


def bcq_pretrain_device_sampled(agent, seed=0):
    """bcq_behavior_pretrain on device-drawn rows -> list of the per-epoch cross-entropy losses.  Each epoch's statistic
    is copied device to device into a (num_epochs,) log that is read back once at the end."""
    rb, eng, opt, B = agent.replay_buffer, agent._behavior_engine, agent.behavior_optimizer, agent.batch_size
    ln_a = math.log(agent.action_size)
    var = N.QnetVariant(0, None, None, None, None, 1)                  # td_off: loss = penalty = CE - ln A
    log = torch.zeros(max(agent.num_epochs, 1), dtype=torch.float32, device=eng.device)
    for epoch in range(agent.num_epochs):
        draw = _next_draw(agent, B)
        if agent._exchange.active:
            idx = E.sample_indices(rb.size, B, seed, draw, device=agent.device)
            _step(agent, eng, opt, rb.gather_device(idx), 1.0, var)
        else:
            m = rb._mirror
            hp = opt.hyper(agent.gamma, 1.0, 1.0 / B)
            args = (m["states"], m["actions"], m["rewards"], m["next_states"], m["dones"])
            if eng.can_sample:
                eng.learn_sampled(hp, *args, rb.size, B, seed, draw, variant=var)
            else:
                idx = E.sample_indices(rb.size, B, seed, draw, device=agent.device)
                eng.learn_indexed(hp, *args, idx, variant=var)
            opt.step_count = hp.step
        log[epoch:epoch + 1].copy_(eng.stats[2:3])
    return [v + ln_a for v in log[:agent.num_epochs].tolist()]
