"""The roll-out evaluators `evaluate_iql`, `evaluate_por`, `evaluate_rvs` (porl_amd/util/util.py) against what the
reference's unmodified loops and policies returned on the scripted environment (tests/golden/evaluate_loops.npz, written
by tests/helpers/gen_normalize_golden.py): the observations do not depend on the action, so an action error of one step
cannot grow in the next.  Per-step actions at the project's forward bar rtol = atol = 1e-5, total reward at rtol 1e-5."""
import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from helpers import normalize_cases as NC
from porl_amd.agent.policy import GaussianPolicy
from porl_amd.dataloader import Normalizer
from porl_amd.util import util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S, A, H, L = NC.EVAL_S, NC.EVAL_A, NC.EVAL_H, NC.EVAL_L
SHAPES = {"iql/policy": (S, A), "por/goal_policy": (S, S), "por/policy": (2 * S, A), "rvs/policy": (S + 2, A)}


@pytest.fixture(scope="module")
def golden():
    z, _ = load_golden("evaluate_loops")
    np.testing.assert_array_equal(z["observations"], NC.eval_observations())      # the fixture holds the helper's script
    m, s = NC.eval_mean_std()
    np.testing.assert_array_equal(z["mean"], m)
    np.testing.assert_array_equal(z["std"], s)
    assert tuple(z["target_goal"]) == NC.EVAL_GOAL
    return z


def _policy(z, name):
    pol = GaussianPolicy(*SHAPES[name], H, L)
    pol.load_state_dict({k: torch.from_numpy(v) for k, v in sub(z, name + "/").items()})
    return pol.to(DEV)


def _run(z, name, deterministic, mean, std):
    env = NC.ScriptedEnv(z["observations"])
    if name == "iql":
        total = U.evaluate_iql(env, _policy(z, "iql/policy"), mean, std, deterministic=deterministic)
    elif name == "por":
        total = U.evaluate_por(env, _policy(z, "por/policy"), _policy(z, "por/goal_policy"), mean, std, deterministic=deterministic)
    else:
        total = U.evaluate_rvs(env, _policy(z, "rvs/policy"), mean, std, deterministic=deterministic)
    return env, total


@pytest.mark.parametrize("name", ("iql", "por", "rvs"))
def test_deterministic_loop_matches_the_reference(golden, name, capsys):
    z = golden
    env, total = _run(z, name, True, z["mean"], z["std"])
    want = z[f"{name}/actions"]
    assert len(env.actions) == NC.EVAL_STEPS == want.shape[0] and env.t == NC.EVAL_STEPS
    got = np.stack(env.actions)
    assert got.shape == want.shape == (NC.EVAL_STEPS, A) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want).max()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(total, float(z[f"{name}/total_reward"]), rtol=1e-5)
    assert isinstance(total, float)
    assert capsys.readouterr().out == ""                            # evaluate_rvs does not print
    print(f"{name}: max action error {err:.2e}")
    # a Normalizer in the place of mean (std ignored) gives the same loop: the same numpy arithmetic on the host
    norm = Normalizer(torch.from_numpy(z["mean"]), torch.from_numpy(z["std"])).to(DEV)
    env2, total2 = _run(z, name, True, norm, None)
    np.testing.assert_array_equal(np.stack(env2.actions), got)
    assert total2 == total
    # host tensors are arrays, not a Normalizer (a Tensor has `numpy` and `apply_` too)
    env3, total3 = _run(z, name, True, torch.from_numpy(z["mean"]), torch.from_numpy(z["std"]))
    np.testing.assert_array_equal(np.stack(env3.actions), got)
    assert total3 == total
    with pytest.raises(TypeError, match="std is required"):
        _run(z, name, True, z["mean"], None)


@pytest.mark.parametrize("name", ("iql", "por", "rvs"))
def test_sampling_loop_ends(golden, name):
    z = golden
    torch.manual_seed(0)
    env, total = _run(z, name, False, z["mean"], z["std"])
    got = np.stack(env.actions)
    assert got.shape == (NC.EVAL_STEPS, A) and np.isfinite(got).all() and np.isfinite(total)
    assert not np.allclose(got, z[f"{name}/actions"], atol=1e-3)     # it sampled
