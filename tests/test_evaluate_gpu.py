"""Scoring without a step — POR.evaluate / SORL.evaluate / evaluate_from_replay / evaluate_store — against the
reference's recorded losses (tests/golden/holdout_ref.npz), an fp64 composition of oracle/por_oracle.py, the update
calls themselves, and for non-interference against an agent that never evaluated."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import holdout_cases as HC
from oracle import por_oracle as O                                  # checker only
from porl_amd.agent.por import POR, evaluate_store
from porl_amd.agent.sorl import SORL
from porl_amd.buffer.replay_buffer import PackedReplay
from porl_amd.dataloader import DeviceDataset, EpochLoader, holdout_region
from porl_amd.util.synth import make_rows, split_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HYPER = HC.SCORE_HYPER
NAMES = {"POR": ("vf", "v_target", "goal_policy"), "SORL": ("v_net", "v_tgt", "policy")}


def _agent(kind, S, H, L, ln=False, A=2, max_batch=256, seed=0, max_steps=1000):
    args = SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=L, layer_norm=ln, action_size=A, max_batch=max_batch)
    torch.manual_seed(seed)
    cls = POR if kind == "POR" else SORL
    return cls(args, max_steps, HYPER[kind]["tau"], HYPER[kind]["alpha"], device=DEV)


def _evaluate(agent, batch, S, A):
    s, r, sp, d, a = split_rows(batch, S, A)
    return agent.evaluate(s, sp, r, d) if isinstance(agent, POR) else agent.evaluate(s, a, r, sp, d)


def _update(agent, batch, S, A):
    s, r, sp, d, a = split_rows(batch, S, A)
    return agent.por_residual_update(s, sp, r, d) if isinstance(agent, POR) else agent.update(s, a, r, sp, d)


def _rel(got, want):
    return abs(got - want) / abs(want)


def _oracle_losses(agent, kind, rows, S, A, L, ln):
    """v_loss, g_loss of the agent's current parameters in fp64, from the oracle's building blocks."""
    vf, vt, pol = NAMES[kind]
    P = {k: v.detach().cpu().numpy() for k, v in agent.state_dict().items()}
    s, r, sp, d, a = (x.astype(np.float64) for x in split_rows(rows, S, A))
    O.set_precision(np.float64)
    try:
        t1, t2, _, _ = O.twin_forward(P, vt, sp, L, ln)
        target = r + (1.0 - d) * agent.discount * np.minimum(t1, t2)
        v1, v2, _, _ = O.twin_forward(P, vf, s, L, ln)
        v_loss = sum(float(O.asymmetric_l2(target - v, agent.tau)[0]) for v in (v1, v2)) / 2.0
        adv = target - np.minimum(v1, v2)
        w = np.minimum(np.exp(adv / agent.alpha if kind == "POR" else agent.alpha * adv), O.EXP_ADV_MAX)
        mean, _ = O.mlp_forward(P, pol + ".net", s, L, False, out_act="tanh" if kind == "SORL" else None)
        nll, _, _ = O.gaussian_nll(mean, sp if kind == "POR" else a, P[pol + ".log_std"].astype(np.float64))
        return v_loss, float(np.mean(w * nll))
    finally:
        O.set_precision(np.float32)


@pytest.mark.parametrize("case", [c[0] for c in HC.SCORE_CASES])
def test_losses_equal_the_references(case):
    z, _ = load_golden("holdout_ref")
    _, kind, ln = next(c for c in HC.SCORE_CASES if c[0] == case)
    s = HC.SCORE_SHAPE
    agent = _agent(kind, s["S"], s["H"], s["L"], ln, s["A"], max_batch=64, seed=123)
    prefix = f"score/{case}/sd/"
    agent.load_state_dict({k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)})
    batch = torch.from_numpy(z["score/rows"]).to(DEV)
    want_v, want_g, want_min = z[f"score/{case}/losses"]
    v_loss, g_loss = _evaluate(agent, batch, s["S"], s["A"])
    print(f"{case}: v_loss {v_loss!r} vs {want_v!r} ({_rel(v_loss, want_v):.2e}), g_loss {g_loss!r} vs {want_g!r} "
          f"({_rel(g_loss, want_g):.2e})")
    assert _rel(v_loss, want_v) <= 1e-5 and _rel(g_loss, want_g) <= 1e-5
    assert _rel(agent.last_min_nll, want_min) <= 1e-5
    # the rows of a store give the same numbers: named rows, then all of them
    replay = PackedReplay(z["score/rows"], s["S"], s["A"], DEV)
    idx = torch.arange(s["B"], dtype=torch.int64, device=DEV)
    assert agent.evaluate_from_replay(replay, s["B"], indices=idx) == (v_loss, g_loss) and replay.draws == 0
    whole = evaluate_store(agent, replay)
    assert (whole["v_loss"], whole["g_loss"], whole["n_rows"]) == (v_loss, g_loss, s["B"])
    assert _rel(whole["min_nll"], want_min) <= 1e-5
    # v_loss is the pre-update loss the next update on the same batch returns
    v_next, _ = _update(agent, batch, s["S"], s["A"])
    print(f"{case}: next update's v_loss {v_next!r} ({_rel(v_loss, v_next):.2e})")
    assert _rel(v_loss, v_next) <= 1e-6


@pytest.mark.parametrize("kind", ["POR", "SORL"])
def test_losses_equal_the_fp64_oracle_after_updates(kind):
    """S = 60, H = 256, L = 2, B = 256, after two updates: target nets differ from the online ones, Adam has moved
    everything, so a mixed-up net or weight would show."""
    S, H, L, B, A = 60, 256, 2, 256, 2
    agent = _agent(kind, S, H, L, False, A, max_batch=B, seed=3)
    rows = make_rows(3 * B, S, A, seed=11)
    drows = torch.from_numpy(rows).to(DEV)
    for k in range(2):
        _update(agent, drows[k * B:(k + 1) * B], S, A)
    want_v, want_g = _oracle_losses(agent, kind, rows[2 * B:], S, A, L, False)
    v_loss, g_loss = _evaluate(agent, drows[2 * B:], S, A)
    print(f"{kind}: v_loss {v_loss!r} vs {want_v!r} ({_rel(v_loss, want_v):.2e}), g_loss {g_loss!r} vs {want_g!r} "
          f"({_rel(g_loss, want_g):.2e})")
    assert _rel(v_loss, want_v) <= 1e-5 and _rel(g_loss, want_g) <= 1e-5
    v_next, _ = _update(agent, drows[2 * B:], S, A)
    assert _rel(v_loss, v_next) <= 1e-6


def _state(agent):
    agent.flush()
    torch.cuda.synchronize()
    opts = (agent.v_optimizer, agent.goal_policy_optimizer if isinstance(agent, POR) else agent.policy_optimizer)
    sched = agent.goal_lr_schedule if isinstance(agent, POR) else agent.lr_schedule
    return ({k: v.clone() for k, v in agent.state_dict().items()}, [o.state_dict() for o in opts], sched.get_last_lr(),
            [o.step_count for o in opts], sched.last_epoch)


def _same(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, torch.Tensor):
        assert torch.equal(a.cpu().view(torch.int32) if a.dtype == torch.float32 else a.cpu(),
                           b.cpu().view(torch.int32) if b.dtype == torch.float32 else b.cpu())
    else:
        assert a == b, (a, b)


@pytest.mark.parametrize("async_losses", [False, True])
@pytest.mark.parametrize("kind", ["POR", "SORL"])
def test_evaluate_does_not_interfere(kind, async_losses):
    """A: two updates, evaluate on another batch, evaluate_store on a 300-row store, two more updates.  B: the four
    updates.  Every loss, the parameters, both optimizers' state, the schedule: bit for bit the same."""
    S, H, L, B, A = 17, 48, 3, 50, 2
    rows = make_rows(5 * B + 300, S, A, seed=21)
    drows = torch.from_numpy(rows).to(DEV)
    store = PackedReplay(rows[5 * B:], S, A, DEV)
    out = {}
    for who in ("A", "B"):
        agent = _agent(kind, S, H, L, kind == "SORL", A, max_batch=64, seed=9)
        agent.async_losses = async_losses
        losses = []

        def update(k):
            got = _update(agent, drows[k * B:(k + 1) * B], S, A)
            if async_losses:                                        # a view of the statistics buffer: complete after flush
                agent.flush()
                torch.cuda.synchronize()
                got = tuple(got[:2].tolist())
            losses.append(got)

        update(0)
        update(1)
        if who == "A":
            before = _state(agent)
            got = _evaluate(agent, drows[4 * B:5 * B], S, A)
            if async_losses:
                assert isinstance(got, torch.Tensor) and got.shape == (3,)
                torch.cuda.synchronize()
                assert torch.isfinite(got).all()
            else:
                assert all(np.isfinite(got))
            res = evaluate_store(agent, store)
            assert res["n_rows"] == 300 and np.isfinite([res["v_loss"], res["g_loss"], res["min_nll"]]).all()
            assert store.draws == 0
            _same(_state(agent), before)                            # nothing moved across the two calls
        update(2)
        update(3)
        out[who] = (losses, _state(agent))
    assert out["A"][0] == out["B"][0]
    _same(out["A"][1], out["B"][1])


@pytest.mark.parametrize("kind", ["POR", "SORL"])
def test_evaluate_store_is_the_row_weighted_mean(kind):
    S, H, L, A, MB = 17, 48, 3, 2, 64
    agent = _agent(kind, S, H, L, False, A, max_batch=MB, seed=4)
    n = MB + 7
    rows = make_rows(n, S, A, seed=31)
    store = PackedReplay(rows, S, A, DEV)
    drows = torch.from_numpy(rows).to(DEV)
    (v1, g1), (v2, g2) = _evaluate(agent, drows[:MB], S, A), _evaluate(agent, drows[MB:], S, A)
    res = evaluate_store(agent, store)
    assert res["n_rows"] == n
    assert _rel(res["v_loss"], (v1 * MB + v2 * 7) / n) <= 1e-6 and _rel(res["g_loss"], (g1 * MB + g2 * 7) / n) <= 1e-6
    # every row is visited once: the last row alone carries a huge reward
    base = evaluate_store(agent, store, batch_size=16)
    assert _rel(base["v_loss"], res["v_loss"]) <= 1e-5              # another chunking, the same mean to fp32 rounding
    big = rows.copy()
    big[-1, S] = 1e4
    hot = evaluate_store(agent, PackedReplay(big, S, A, DEV))
    rest = evaluate_store(agent, PackedReplay(big[:-1], S, A, DEV))
    last = _evaluate(agent, torch.from_numpy(big[-1:]).to(DEV), S, A)
    assert last[0] > 1e6 and hot["v_loss"] > 1e6 / n
    assert _rel(hot["v_loss"], (rest["v_loss"] * (n - 1) + last[0]) / n) <= 1e-6
    with pytest.raises(RuntimeError, match="max_batch"):
        evaluate_store(agent, store, batch_size=MB + 1)
    with pytest.raises(ValueError, match="no rows"):
        evaluate_store(agent, PackedReplay(rows[:0], S, A, DEV))


def test_from_replay_draws_like_update_from_replay():
    S, H, L, A, B = 17, 48, 3, 2, 32
    rows = make_rows(200, S, A, seed=41)
    agent = _agent("POR", S, H, L, False, A, max_batch=64, seed=5)
    replay = PackedReplay(rows, S, A, DEV, seed=7)
    got = agent.evaluate_from_replay(replay, B)                     # draw 0
    assert replay.draws == 1
    twin = PackedReplay(rows, S, A, DEV, seed=7)
    idx = twin.sample_indices(B).clone()                            # the same draw 0
    assert agent.evaluate_from_replay(replay, B, indices=idx) == got and replay.draws == 1
    batch = torch.from_numpy(rows).to(DEV)[idx]
    assert _evaluate(agent, batch, S, A) == got
    replay.draws = 0
    v_next, _ = agent.update_from_replay(replay, B)                 # the update draws the same rows
    assert _rel(got[0], v_next) <= 1e-6
    with pytest.raises(RuntimeError, match="indices"):
        agent.evaluate_from_replay(replay, B, indices=idx[:5])
    with pytest.raises(ValueError, match="wide"):
        agent.evaluate_from_replay(PackedReplay(make_rows(8, 5, A, seed=1), 5, A, DEV), 4)


def test_backbone_is_out_of_scope():
    from porl_amd.agent.fasternet import FasterNet
    torch.manual_seed(0)
    args = SimpleNamespace(state_size=362, feature_dim=32, hidden_dim=32, n_hidden=1, layer_norm=False, action_size=2,
                           max_batch=8)
    agent = SORL(args, 10, 0.9, 3.0, device=DEV, backbone=FasterNet(3, 32))
    x, v = torch.zeros(2, 362, device=DEV), torch.zeros(2, device=DEV)
    replay = PackedReplay(np.zeros((4, 2 * 362 + 4), dtype=np.float32), 362, 2, DEV)
    for call in (lambda: agent.evaluate(x, torch.zeros(2, 2, device=DEV), v, x, v),
                 lambda: agent.evaluate_from_replay(replay, 2), lambda: evaluate_store(agent, replay)):
        with pytest.raises(NotImplementedError, match="backbone"):
            call()
    assert replay.draws == 0


def test_end_to_end_train_without_a_region_and_score_it():
    S, H, L, A, B = 17, 48, 3, 2, 64
    rows = make_rows(4096, S, A, seed=51)
    rng = np.random.default_rng(52)
    rows[:, 0], rows[:, 1] = rng.uniform(0, 10, 4096), rng.uniform(0, 10, 4096)
    replay = PackedReplay(rows, S, A, DEV, seed=3)
    train, held = holdout_region(replay, x_range=(2, 5), y_range=(3, 8))
    m = HC.held_mask(rows, (2, 5), (3, 8))
    assert len(held) == m.sum() > 200 and len(train) == 4096 - m.sum()
    agent = _agent("SORL", S, H, L, False, A, max_batch=B, seed=6)
    first = evaluate_store(agent, held)
    for _ in range(20):
        v_loss, g_loss = agent.update_from_replay(train, B)
        assert np.isfinite(v_loss) and np.isfinite(g_loss)
    assert train.draws == 20 and held.draws == 0
    res = evaluate_store(agent, held)
    assert res["n_rows"] == len(held) and np.isfinite([res["v_loss"], res["g_loss"], res["min_nll"]]).all()
    assert res["v_loss"] != first["v_loss"]                         # the parameters have moved, the held-out score with them
    loader = EpochLoader(DeviceDataset.from_tensor(held.rows), 100)
    seen = torch.cat(list(loader))
    assert seen.shape == held.rows.shape
    assert torch.equal(seen.sum(dim=0, dtype=torch.float64), held.rows.sum(dim=0, dtype=torch.float64))
