"""The goal-conditioned behaviour-cloning cases (tests/helpers/bc_cases.py) on the CPU: the pools hold what the grid
needs, the inputs are what their description says, and the numpy restatement of the step reproduces the golden recorded
from the reference's own unmodified method (tests/helpers/gen_goal_bc_golden.py).  No device use."""
import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from helpers import bc_cases as BCC
from oracle import por_oracle as O
from porl_amd.util.synth import make_rows, split_rows

GOLDEN = "goal_bc_s60_h64_b32"
LOSS_RTOL, PARAM_ATOL = 2e-5, 1e-5          # the bounds of tests/test_sorl_phases_gpu.py against a reference golden


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    O.set_precision(np.float32)


def test_grid_is_the_one_the_issue_sets():
    got = [(c.S, c.G, c.goal_col, c.A, c.H, c.L, int(c.tanh)) for c in BCC.CONFIGS]
    assert got == [(60, 60, 61, 2, 48, 2, 0), (60, 2, 0, 2, 132, 2, 1), (3, 1, 4, 1, 30, 1, 1), (17, 17, 0, 6, 48, 3, 0),
                   (182, 182, 183, 2, 48, 2, 0)]
    for c in BCC.CONFIGS:
        want = {1, 9, 65, 130} | ({1030} if c is BCC.CONFIGS[0] else set())
        assert {B for n, B in BCC.RUNS if n == c.name} == want
        assert c.goal_col >= 0 and c.goal_col + c.G <= 2 * c.S + 2         # the goal lies in the state part of a row


@pytest.mark.parametrize("name", [c.name for c in BCC.CONFIGS])
def test_every_pool_yields_its_largest_batch_of_decided_rows(name):
    cfg, P = BCC.params(name)
    p = BCC.pool(name)
    B = BCC.max_batch_of(name)
    print(f"{name}: {p['n_decided']} decided rows of {p['n_pool']}, largest batch {B}")
    assert p["n_decided"] >= B
    x, a = BCC.batch(name, B)
    assert x.shape == (B, cfg.S + cfg.G) and a.shape == (B, cfg.A) and x.dtype == a.dtype == np.float32
    # decided means decided: every hidden pre-activation of the batch is at least MARGIN from zero in fp64
    O.set_precision(np.float64)
    P64 = {k: v.astype(np.float64) for k, v in P.items()}
    for z in BCC.BC._preacts(P64, BCC.PREFIX + ".net", x.astype(np.float64), cfg.L, False):
        assert np.abs(z).min() >= BCC.MARGIN
    # the stored actions sit at |z| in [0.4, 1.6] of the fp64 mean
    mean, _ = O.mlp_forward(P64, BCC.PREFIX + ".net", x.astype(np.float64), cfg.L, False, "tanh" if cfg.tanh else None)
    O.set_precision(np.float32)
    sigma = np.exp(np.clip(P64[BCC.PREFIX + ".log_std"], O.LOG_STD_MIN, O.LOG_STD_MAX))
    z = np.abs((a.astype(np.float64) - mean) / sigma)
    ulp = np.spacing(np.abs(a)).astype(np.float64) / sigma                 # the action was rounded to fp32
    assert (z >= 0.4 - ulp).all() and (z <= 1.6 + ulp).all()
    # the pairs: start rows are distinct, goal rows lie in the store, and goal == start occurs where the goal is another row's state
    start, goal = BCC.pairs(name, B)
    assert len(set(start.tolist())) == B and goal.min() >= 0 and goal.max() < p["n_pool"]
    if cfg.goal_col == cfg.S + 1:
        assert (goal == start).all()
    elif B >= 65:
        assert (goal == start).any() and (goal != start).any()


def test_log_std_entries_sit_on_inside_and_outside_the_clamp():
    seen = set()
    for c in BCC.CONFIGS:
        ls = BCC.log_std_for(c)
        assert ls.shape == (c.A,)
        seen |= {float(v) for v in ls if float(v) in BCC.BC.LS_SPECIAL}
        if c.A >= 4:
            assert set(BCC.BC.LS_SPECIAL) <= {float(v) for v in ls}
            assert any(-5.0 < v < 2.0 for v in ls)
    assert seen == set(BCC.BC.LS_SPECIAL)
    inside = [v for c in BCC.CONFIGS for v in BCC.log_std_for(c) if -5.0 < v < 2.0]
    assert inside


def test_clamped_entries_have_zero_gradient_and_the_bar_rule_is_forward_cases():
    name = BCC.CONFIGS[3].name
    ref = BCC.reference(name, 9)
    out = BCC.clamped_out(name)
    assert len(out) == 2
    assert (ref["ref"]["grads"][BCC.PREFIX + ".log_std"][out] == 0).all()
    assert (np.delete(ref["ref"]["grads"][BCC.PREFIX + ".log_std"], out) != 0).all()
    assert BCC.BAR_FLOOR == 2e-6 and BCC.BAR_FACTOR == 4.0
    for k, e in ref["e32"].items():
        assert ref["bar"][k] == max(2e-6, 4.0 * e)
        assert e < 1e-4, (k, e)                                           # the fp32 restatement is a sane yardstick for the bar


def test_fp64_gradients_match_finite_differences():
    """The restatement's gradient is the gradient of the restated loss (central differences in fp64)."""
    name = BCC.CONFIGS[2].name
    cfg, P = BCC.params(name)
    x, a = BCC.batch(name, 9)
    ref = BCC.bc_grads(cfg, P, x, a, np.float64)
    rng = np.random.default_rng(5)
    for key in BCC.param_names(cfg):
        for _ in range(3):
            idx = tuple(rng.integers(0, s) for s in P[key].shape)
            h = 1e-6
            vals = []
            for sgn in (1.0, -1.0):
                Q = {k: v.astype(np.float64) for k, v in P.items()}
                Q[key][idx] += sgn * h
                vals.append(float(BCC.bc_grads(cfg, Q, x, a, np.float64)["stats"][0]))
            fd = (vals[0] - vals[1]) / (2 * h)
            g = float(ref["grads"][key][idx])
            if key.endswith("log_std") and idx[0] in BCC.clamped_out(name):
                assert g == 0.0
            elif key.endswith("log_std") and float(P[key][idx]) in (-5.0, 2.0):
                # exactly on an end of the clamp: torch's clamp passes the gradient (the oracle's `inside` is inclusive),
                # while the loss is flat on the far side, so the central difference sees half the slope
                assert abs(fd - g / 2) <= 1e-6 * max(1.0, abs(g)), (key, idx, fd, g)
            else:
                assert abs(fd - g) <= 1e-6 * max(1.0, abs(g)), (key, idx, fd, g)


def test_restatement_reproduces_the_reference_golden():
    """Five steps of the fp32 restatement from the golden's initial parameters, on rows made from the recorded seed."""
    z, meta = load_golden(GOLDEN)
    S, G, H, L, B, K, A = (int(meta[k]) for k in ("S", "G", "H", "L", "B", "K", "A"))
    assert (S, G, H, L, B, K, A) == (60, 60, 64, 2, 32, 5, 2)
    cfg = BCC.Config("golden", S, G, S + 1, A, H, L, False)
    o = BCC.BcOracle(cfg, sub(z, "init/"), np.float32, lr0=meta["policy_lr"], t_max=int(meta["max_steps"]))
    rows = make_rows(K * B, S, A, seed=int(meta["seed_data"]))
    for k in range(K):
        blk = rows[k * B:(k + 1) * B]
        start = np.arange(B)
        x, a = BCC.gather_inputs(cfg, blk, start, start)
        s, _, sp, _, act = split_rows(blk, S, A)
        assert np.array_equal(x, np.concatenate([s, sp], axis=1)) and np.array_equal(a, act)
        loss = o.update(x, a)
        print(f"policy_loss[{k}] = {loss!r} (reference {float(z['policy_loss'][k])!r})")
        np.testing.assert_allclose(loss, z["policy_loss"][k], rtol=LOSS_RTOL)
    final, adam = sub(z, "final/"), sub(z, "adam/")
    for n in BCC.param_names(cfg):
        assert float(np.abs(o.P[n].astype(np.float64) - final[n]).max()) <= PARAM_ATOL, n
        assert float(np.abs(o.adam.m[n].astype(np.float64) - adam[n + ".exp_avg"]).max()) <= PARAM_ATOL, n
        assert float(np.abs(o.adam.v[n].astype(np.float64) - adam[n + ".exp_avg_sq"]).max()) <= PARAM_ATOL, n
    assert int(adam["__step__"]) == K
    np.testing.assert_allclose(O.cosine_lr(meta["policy_lr"], K, int(meta["max_steps"])), z["last_lr"][0], rtol=1e-12)


def test_seeded_initialisation_is_the_reference_one_bit_for_bit():
    """The constructor consumes the seeded generator as the reference's GaussianPolicy(2S, A) does."""
    from porl_amd.agent import GoalConditionedBC
    z, meta = load_golden(GOLDEN)
    torch.manual_seed(int(meta["seed_model"]))
    bc = GoalConditionedBC(int(meta["S"]), int(meta["G"]), int(meta["A"]), int(meta["max_steps"]),
                           hidden_dim=int(meta["H"]), n_hidden=int(meta["L"]), max_batch=int(meta["B"]))
    sd = bc.state_dict()
    init = sub(z, "init/")
    assert list(sd.keys()) == list(init.keys()) == BCC.param_names(BCC.Config("g", 60, 60, 61, 2, 64, 2, False))
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), init[k]), k
    assert bc.policy_lr_schedule.T_max == int(meta["max_steps"]) and bc.policy_optimizer.lr == meta["policy_lr"]
