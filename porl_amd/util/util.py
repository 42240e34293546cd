"""Builder helpers with the reference's module structure (so state_dict keys interchange).

Mirrors the *interface* of /root/reference/util/util.py:20-56 (`Squeeze`, `mlp`,
`update_exponential_moving_average`); the modules built here only carry parameters and shapes —
device arithmetic is done by the HIP engine (porl_amd/engine.py), never by torch.nn.functional.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn


class Squeeze(nn.Module):
    """Marker module: drop a singleton dimension (reference util/util.py:20-26)."""

    def __init__(self, dim=None):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        return x.squeeze(dim=self.dim)


def mlp(dims, activation=nn.ReLU, output_activation=None, layer_norm=False, squeeze_output=False):
    """Linear [-> LayerNorm] -> act, repeated; then Linear [-> out act] [-> Squeeze(-1)].

    Same positional layout inside nn.Sequential as the reference (util/util.py:29-47), hence the same
    parameter names ('0.weight', '2.weight', ... or '0','1','3','4',... with layer_norm) and the same
    consumption of the torch RNG at construction.
    """
    if len(dims) < 2:
        raise AssertionError("MLP requires at least two dims (input and output)")
    mods = []
    for fan_in, fan_out in zip(dims[:-2], dims[1:-1]):
        mods.append(nn.Linear(fan_in, fan_out))
        if layer_norm:
            mods.append(nn.LayerNorm(fan_out))
        mods.append(activation())
    mods.append(nn.Linear(dims[-2], dims[-1]))
    if output_activation is not None:
        mods.append(output_activation())
    if squeeze_output:
        if dims[-1] != 1:
            raise AssertionError("squeeze_output needs a scalar head")
        mods.append(Squeeze(-1))
    return nn.Sequential(*mods).to(dtype=torch.float32)


def mlp_spec(seq: nn.Sequential):
    """Decode an `mlp()` Sequential into (dims, layer_norm, out_act) for the engine."""
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    dims = [lin[0].in_features] + [m.out_features for m in lin]
    layer_norm = any(isinstance(m, nn.LayerNorm) for m in seq)
    out_act = "tanh" if any(isinstance(m, nn.Tanh) for m in seq) else None
    return dims, layer_norm, out_act


def update_exponential_moving_average(target, source, alpha):
    """target <- (1-alpha)*target + alpha*source (reference util/util.py:54-56), stand-alone (the training step fuses
    this into the Adam sweep).  Device tensors go through the `porl_ema` kernel when they are 16-byte aligned and a
    multiple of 4 floats long (every weight matrix and hidden bias of the engines' flat groups); odd-sized leftovers
    (a scalar head bias) and CPU modules use the two torch ops of the reference."""
    from .. import engine as E
    with torch.no_grad():
        for t, s in zip(target.parameters(), source.parameters()):
            if (t.is_cuda and s.is_cuda and t.is_contiguous() and s.is_contiguous() and t.dtype == torch.float32
                    and t.numel() % 4 == 0 and t.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0):
                E.ema(t, s, alpha)
            else:
                t.mul_(1.0 - alpha).add_(s, alpha=alpha)


def extract_done_makers(dones):
    """Episode table (starts, ends, lengths) of a done-flag vector (reference util/util.py:83-87), on the device:
    porl_amd.dataloader.episodes.extract_done_makers."""
    from ..dataloader import episodes
    return episodes.extract_done_makers(dones)


def return_range(dataset, max_episode_steps):
    """(min, max) episode return (reference util/util.py:67-80), on the device:
    porl_amd.dataloader.episodes.return_range."""
    from ..dataloader import episodes
    return episodes.return_range(dataset, max_episode_steps)


def rvs_sample_batch(dataset, batch_size):
    """Hindsight-goal minibatch (reference util/util.py:129-138) from a PackedReplay, on the device:
    porl_amd.dataloader.episodes.rvs_sample_batch."""
    from ..dataloader import episodes
    return episodes.rvs_sample_batch(dataset, batch_size)


def generate_test_generlaization_data(dataset, env_name, env_idx=None):
    """Delete the transitions inside the hold-out box of `env_name` (reference util/util.py:219-238, its spelling), on
    the device: porl_amd.dataloader.holdout.generate_test_generlaization_data."""
    from ..dataloader import holdout
    return holdout.generate_test_generlaization_data(dataset, env_name, env_idx)


def torchify(x, device):
    """A host array as a tensor on `device`, fp64 narrowed to fp32 (the reference's helper of this name, util/util.py:59-64,
    sends it to a global `DEFAULT_DEVICE` that it never defines; the evaluators below pass the policy's device)."""
    t = torch.as_tensor(np.asarray(x))
    return t.to(device=device, dtype=torch.float32 if t.dtype == torch.float64 else t.dtype)


def _host_stats(what, mean, std, nets):
    """(mean, std) as host arrays and the device of `nets`.  `mean` may be a dataloader.Normalizer, which carries both
    (`std` is then ignored).  There is no CPU path: a network on the host raises NativeError."""
    from .. import _native as N
    from ..dataloader.normalize import Normalizer
    devices = [next(net.parameters()).device for net in nets]
    for d in devices:
        if d.type != "cuda":
            raise N.NativeError(f"{what}: the policy is on {d}, policy.act runs on a HIP device only (no CPU path)")
    if isinstance(mean, Normalizer):
        mean, std = mean.numpy()
    elif std is None:
        raise TypeError(f"{what}: std is required unless mean is a Normalizer")
    return np.asarray(mean), np.asarray(std), devices[0]


def _rollout(env, policy, mean, std, device, deterministic, begin):
    """One episode, the sum of its rewards.  Per step, in the reference's order (util/util.py:141-185): the observation
    is normalised in numpy on the host, `step_input` turns it into the policy's input, the policy acts on the device
    and the environment (four return values) takes the action.  `begin(act)` runs once after `env.reset()` and returns
    `step_input`; `act(net, x)` is a network's action for the host vector `x`, back on the host."""
    def act(net, x):
        with torch.no_grad():
            return net.act(torchify(x, device), deterministic=deterministic).cpu().numpy()

    raw = env.reset()
    step_input = begin(act)
    episode_return, finished = 0.0, False
    while not finished:
        raw, reward, finished, _ = env.step(act(policy, step_input((raw - mean) / std)))
        episode_return += reward
    return episode_return


def evaluate_iql(env, policy, mean, std=None, deterministic=True):
    """Return of one episode of `policy` on normalised observations.  `mean, std` are numpy arrays, or `mean` is a
    dataloader.Normalizer."""
    mean, std, device = _host_stats("evaluate_iql", mean, std, (policy,))
    return _rollout(env, policy, mean, std, device, deterministic, lambda act: lambda z: z)


def evaluate_por(env, policy, goal_policy, mean, std=None, deterministic=True):
    """Return of one episode in which `goal_policy` proposes a goal from the normalised observation and `policy` acts on
    [observation | goal]."""
    mean, std, device = _host_stats("evaluate_por", mean, std, (policy, goal_policy))
    return _rollout(env, policy, mean, std, device, deterministic,
                    lambda act: lambda z: np.concatenate([z, act(goal_policy, z)]))


def evaluate_rvs(env, policy, mean, std=None, deterministic=True):
    """Return of one episode in which `policy` acts on [observation | goal]: the goal is `env.target_goal`, read once
    after the reset and normalised by the first two entries of `mean, std`.  The reference's progress print is left
    out."""
    mean, std, device = _host_stats("evaluate_rvs", mean, std, (policy,))

    def begin(act):
        goal = (np.asarray(env.target_goal) - mean[:2]) / std[:2]
        return lambda z: np.concatenate([z, goal])

    return _rollout(env, policy, mean, std, device, deterministic, begin)
