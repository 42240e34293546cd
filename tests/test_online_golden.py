"""CPU checks of the train_online fixtures (scripts/gen_golden_online.py) and of the toy environment they were made on:
the fixtures must exercise what tests/test_online_gpu.py claims from them."""
import numpy as np
import pytest

from conftest import load_golden, sub
from helpers.online_env import RecordingLogger, ToyEnv


@pytest.mark.parametrize("kind", ["dqn", "ddqn", "c51"])
def test_online_fixture_is_meaningful(kind):
    z, _ = load_golden(f"online_{kind}_s8_a4")
    S, A, EP, MS, THR, B, TF, CAP, seed_env, seed_np, atoms = (int(v) for v in z["meta"])
    assert (S, A) == (8, 4)
    assert float(z["min_gap"]) > 1e-3 and int(z["n_greedy"]) > 10
    ends = z["ends"]
    assert len(ends) == EP and ends.any() and not ends.all()       # episodes end by termination and by truncation
    n = len(z["actions"])
    assert len(z["losses"]) == n - THR + 1                            # one learn per step from the threshold on
    assert int(z["log_calls"][:, 3].sum()) == len(z["losses"])
    assert len(z["buf/states"]) == n and np.isfinite(z["losses"]).all()
    assert set(sub(z, "init/")) == set(sub(z, "final/")) == set(sub(z, "final_target/"))


def test_toy_env_is_deterministic_and_leaves_the_global_stream_alone():
    np.random.seed(4)
    before = np.random.get_state()[1].copy()
    runs = []
    for _ in range(2):
        env = ToyEnv(seed=2)
        s, info = env.reset()
        out = [s]
        for a in [0, 1, 2, 3] * 10:
            s, r, term, trunc, _ = env.step(a)
            out += [s, np.float32(r)]
            if term or trunc:
                out.append(env.reset()[0])
        runs.append(np.concatenate([np.ravel(o) for o in out]))
        assert s.dtype == np.float32 and info == {}
    np.testing.assert_array_equal(runs[0], runs[1])
    assert (np.random.get_state()[1] == before).all()
    log = RecordingLogger()
    log.log_step(0, 1, 0.5, None, 1.0)
    assert log.calls == [("log_step", 0, 1, 0.5, None, 1.0)]
