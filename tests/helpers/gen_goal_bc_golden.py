#!/usr/bin/env python3
"""Golden fixture of the goal-conditioned action policy's update (tests/golden/goal_bc_s60_h64_b32.npz).  TEST
INFRASTRUCTURE — runs only where the reference implementation is importable (CPU); its output, a small .npz data file, is
all that travels.

The update is live text of the reference, agent/por.py:178-184, inside `POR.por_qlearning_update`.  That method reads four
attributes `POR.__init__` never sets (their assignments are commented out at por.py:60-63, `b_goal_policy` is set by
`pretrain_init`, which needs an undefined global): `policy`, `policy_optimizer`, `policy_lr_schedule`, `b_goal_policy`.
This generator supplies the four from OUTSIDE, built with the reference's own classes and the arguments of the
commented-out lines, and then runs the UNMODIFIED method; `wandb` is only named at step 100 000.  The action-policy part
of the method depends on nothing else in it (checked: its parameters after the run are bit-identical to the six
statements of :178-184 run stand-alone), so what is recorded is the reference's own result for that block.  Nothing of
the reference is edited or copied.

Recorded: meta_*, init/ and final/ (the action policy's state dict under the prefix `policy.`), adam/ (its Adam state),
policy_loss (K values, recomputed from the pre-update parameters by the reference's own modules, since the method returns
nothing), last_lr.  Rows: make_rows(K * B, S, A, seed_data), batch k = rows[k*B:(k+1)*B], goal = s' (por.py:178).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/helpers/gen_goal_bc_golden.py </dev/null
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from oracle.gen_golden import OUT, adam_np, pack, sd_np  # noqa: E402  (puts the reference on sys.path)
from porl_amd.util.synth import make_rows, split_rows  # noqa: E402


def gen(name, S, H, L, B, K, A=2, seed_model=0, seed_data=4, max_steps=1000, policy_lr=1e-4):
    from agent.policy import GaussianPolicy
    from agent.por import POR
    from torch.optim.lr_scheduler import CosineAnnealingLR
    args = SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=L, layer_norm=False, feature_dim=256, action_size=A)
    torch.manual_seed(seed_model)
    # the action policy is built FIRST, so that its initialisation is the first consumer of the seeded generator: the
    # drop-in's constructor reproduces it from seed_model alone
    policy = GaussianPolicy(2 * S, A, hidden_dim=H, n_hidden=L)
    agent = POR(args, max_steps, 0.9, 10.0)
    agent.policy = policy                                                       # por.py:60
    agent.policy_optimizer = torch.optim.Adam(agent.policy.parameters(), lr=policy_lr)      # por.py:62
    agent.policy_lr_schedule = CosineAnnealingLR(agent.policy_optimizer, max_steps)         # por.py:63
    agent.b_goal_policy = GaussianPolicy(S, S, hidden_dim=H, n_hidden=L)        # pretrain_init's attribute
    rows = make_rows(K * B, S, A, seed=seed_data)
    init = sd_np(agent.policy)
    losses = []
    for k in range(K):
        s, r, sp, d, a = split_rows(torch.from_numpy(rows[k * B:(k + 1) * B]), S, A)
        with torch.no_grad():
            losses.append(float((-agent.policy(torch.concat([s, sp], dim=1)).log_prob(a)).mean()))
        torch.manual_seed(1000 + k)                                             # goal_out.rsample() draws; not ours
        agent.por_qlearning_update(s, a, sp, r, d)
    final = sd_np(agent.policy)
    meta = dict(S=S, G=S, H=H, L=L, B=B, K=K, A=A, seed_model=seed_model, seed_data=seed_data, max_steps=max_steps,
                policy_lr=policy_lr)
    out = {"meta_" + k: np.float64(v) for k, v in meta.items()}
    out["policy_loss"] = np.array(losses, dtype=np.float64)
    out["last_lr"] = np.array(agent.policy_lr_schedule.get_last_lr(), dtype=np.float64)
    out.update(pack("init/policy.", init))
    out.update(pack("final/policy.", final))
    names = [n for n, _ in agent.policy.named_parameters(prefix="policy")]
    out.update(pack("adam/", adam_np(agent.policy_optimizer, names)))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: policy_loss={losses} last_lr={out['last_lr']} step={agent.step}")


if __name__ == "__main__":
    gen("goal_bc_s60_h64_b32", S=60, H=64, L=2, B=32, K=5)
