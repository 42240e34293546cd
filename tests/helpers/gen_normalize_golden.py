"""Writes tests/golden/evaluate_loops.npz: what the reference's roll-out evaluators return on the scripted environment.

    python tests/helpers/gen_normalize_golden.py <reference_dir>

Runs on a CPU box with the reference checked out; never on the GPU machine.  The reference's unmodified `evaluate_iql`,
`evaluate_por` and `evaluate_rvs` (util/util.py:141-185) are imported and run with its own `GaussianPolicy`
(agent/policy.py:12-33), seeded; `DEFAULT_DEVICE`, which util/util.py uses without defining, is supplied as a module
global (the CPU).  The environment is normalize_cases.ScriptedEnv: a recorded observation sequence independent of the
action, reward -|a|^2, done at step 12.  Recorded: the observations, mean / std, every policy's state_dict, the actions
of every step and the total reward, all for deterministic=True.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import normalize_cases as NC  # noqa: E402

if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
OUT = os.path.join(os.path.dirname(HERE), "golden", "evaluate_loops.npz")


def main():
    sys.path.insert(0, REF)
    from agent.policy import GaussianPolicy
    from util import util as U
    U.DEFAULT_DEVICE = torch.device("cpu")
    S, A, H, L = NC.EVAL_S, NC.EVAL_A, NC.EVAL_H, NC.EVAL_L
    mean, std = NC.eval_mean_std()
    z = {"observations": NC.eval_observations(), "mean": mean, "std": std, "target_goal": np.array(NC.EVAL_GOAL)}
    torch.manual_seed(0)
    nets = {"iql/policy": GaussianPolicy(S, A, H, L), "por/goal_policy": GaussianPolicy(S, S, H, L),
            "por/policy": GaussianPolicy(2 * S, A, H, L), "rvs/policy": GaussianPolicy(S + 2, A, H, L)}
    with torch.no_grad():
        for net in nets.values():                                  # log_std is zeros at construction: make it matter
            net.log_std.copy_(torch.randn(net.log_std.shape) * 0.3)
    for name, net in nets.items():
        for k, v in net.state_dict().items():
            z[f"{name}/{k}"] = v.detach().numpy()
    runs = {"iql": lambda e: U.evaluate_iql(e, nets["iql/policy"], mean, std),
            "por": lambda e: U.evaluate_por(e, nets["por/policy"], nets["por/goal_policy"], mean, std),
            "rvs": lambda e: U.evaluate_rvs(e, nets["rvs/policy"], mean, std)}
    for name, run in runs.items():
        env = NC.ScriptedEnv()
        with contextlib.redirect_stdout(io.StringIO()):            # evaluate_rvs prints its location
            total = run(env)
        z[f"{name}/actions"] = np.stack(env.actions)
        z[f"{name}/total_reward"] = np.array(total, dtype=np.float64)
        print(f"{name}: {len(env.actions)} steps, total reward {total:.8f}")
    np.savez_compressed(OUT, **z)
    print(f"-> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
