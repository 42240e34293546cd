#!/usr/bin/env python3
"""Golden fixtures of two-phase SORL training (tests/golden/sorl_2phase_*.npz).  TEST INFRASTRUCTURE — runs only where
the reference implementation is importable (CPU); its output, small .npz data files, is all that travels.

The reference's two-phase script (sorl_train_v0.py:57-103) runs `SORL.vf_update` for the value epochs and then
`SORL.policy_update` with the value nets frozen.  Upstream `policy_update` (agent/sorl.py:154-176) reads a name,
`target_v`, that it never assigns (NameError, sorl.py:163); the two lines that assign it stand verbatim in `update` and
`vf_update` of the same file (sorl.py:85-89).  This generator supplies exactly those two lines from OUTSIDE: before
each call it computes `target_v` with the reference agent's own `v_tgt` and stores it as a global of the reference's
`agent.sorl` module, where the unmodified method then finds it.  Nothing of the reference is edited.

Recorded: meta_*, init/, v_loss (KV value steps), g_loss (KP policy steps), mid/ (state after phase one), final/,
both Adam states, the cosine schedule's get_last_lr() after the run.  Rows: make_rows((KV + KP) * B, S, A, seed_data),
batch k = rows[k*B:(k+1)*B], value steps first.

Usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_sorl_phases.py </dev/null
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from oracle.gen_golden import OUT, adam_np, pack, sd_np  # noqa: E402
from porl_amd.util.synth import make_rows, split_rows  # noqa: E402


def gen(name, S, H, L, layer_norm, B, KV, KP, A=2, alpha=3.0, tau=0.9, seed_model=0, seed_data=2, max_steps=1000):
    import agent.sorl as ref_sorl
    args = SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=L, layer_norm=layer_norm, feature_dim=256, action_size=A)
    torch.manual_seed(seed_model)
    agent = ref_sorl.SORL(args, max_steps, tau, alpha)
    rows = make_rows((KV + KP) * B, S, A, seed=seed_data)
    init = sd_np(agent)
    v_losses, g_losses = [], []
    for k in range(KV):
        s, r, sp, d, a = split_rows(torch.from_numpy(rows[k * B:(k + 1) * B]), S, A)
        v_losses.append(agent.vf_update(s, a, r, sp, d))
    mid = sd_np(agent)
    for k in range(KV, KV + KP):
        s, r, sp, d, a = split_rows(torch.from_numpy(rows[k * B:(k + 1) * B]), S, A)
        with torch.no_grad():                                    # sorl.py:85-89, the two lines policy_update lacks
            next_v = agent.v_tgt(sp)
        ref_sorl.target_v = r + (1. - d.float()) * agent.discount * next_v
        g_losses.append(agent.policy_update(s, a, r, sp, d))
    del ref_sorl.target_v
    final = sd_np(agent)
    meta = dict(S=S, H=H, L=L, layer_norm=int(layer_norm), B=B, KV=KV, KP=KP, A=A, seed_model=seed_model,
                seed_data=seed_data, tau=tau, alpha=alpha, max_steps=max_steps, discount=0.99, beta=0.005,
                value_lr=1e-4, policy_lr=1e-4)
    out = {"meta_" + k: np.float64(v) for k, v in meta.items()}
    out["v_loss"] = np.array(v_losses, dtype=np.float64)
    out["g_loss"] = np.array(g_losses, dtype=np.float64)
    out["last_lr"] = np.array(agent.lr_schedule.get_last_lr(), dtype=np.float64)
    out["keys"] = np.array(list(final.keys()))
    out.update(pack("init/", init))
    out.update(pack("mid/", mid))
    out.update(pack("final/", final))
    v_names = [n for n, _ in agent.v_net.named_parameters(prefix="v_net")]
    p_names = [n for n, _ in agent.policy.named_parameters(prefix="policy")]
    out.update(pack("adam_v/", adam_np(agent.v_optimizer, v_names)))
    out.update(pack("adam_g/", adam_np(agent.policy_optimizer, p_names)))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: v_loss={v_losses} g_loss={g_losses} last_lr={out['last_lr']}")


def main():
    gen("sorl_2phase_s60_h64_b32", S=60, H=64, L=2, layer_norm=False, B=32, KV=3, KP=4)
    gen("sorl_2phase_s60_h64_b32_ln", S=60, H=64, L=2, layer_norm=True, B=32, KV=3, KP=4)


if __name__ == "__main__":
    main()
