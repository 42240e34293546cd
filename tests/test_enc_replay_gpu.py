"""`update_from_replay` with a backbone and with `indices=`: rows of a device-resident PackedReplay are encoded where they
lie (`FasterNet.forward_rows` -> porl_enc_forward_rows) and staged by index (porl_iql_load_batch_indexed); the store is
only read.  The extension's arithmetic is defined as "what the tensor form computes on those rows", so it is checked

  1. against the two reference goldens that exist for backbone agents (bounds: those of tests/test_fasternet_gpu.py,
     measured against the reference and accepted for these goldens),
  2. bit for bit against `gather` + `split` + the tensor form, values > 8 planted in the store (the tensor form zeroes
     them in its copy, the row form must read them as 0 and leave the store alone),
  3. bit for bit for `indices=` without a backbone, and for the unchanged device draw,
  4. on the first and last row of the store, named twice,
  5. through its refusals, which launch and count nothing,
  6. through the data-parallel branch, on a forced one-rank exchange.

GPU only.  Small shapes: FasterNet(3, 256, max_batch=8), heads H=64 L=2, stores of 23 rows."""
import json
import os
import socket
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def rel_err(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def _replay(rows, S, A, seed=0):
    from porl_amd.buffer.replay_buffer import PackedReplay
    return PackedReplay(rows, S, A, DEV, seed=seed)


def _lidar_rows(N, n_ang, A, seed):
    """[s | r | s' | d | a] rows whose states look like lidar scans: beams in (0.2, 3.9), goal in (-3, 3)^2."""
    rng = np.random.default_rng(seed)
    S = n_ang + 2
    rows = np.empty((N, 2 * S + 2 + A), dtype=np.float32)
    for off in (0, S + 1):
        rows[:, off:off + n_ang] = rng.uniform(0.2, 3.9, size=(N, n_ang))
        rows[:, off + n_ang:off + S] = rng.uniform(-3, 3, size=(N, 2))
    rows[:, S] = rng.normal(size=N)
    rows[:, 2 * S + 1] = rng.uniform(size=N) < 0.2
    rows[:, 2 * S + 2:] = rng.uniform(-1, 1, size=(N, A))
    return rows


def _agent(kind, n_ang, n_dist, A, dtype="fp32", seed=3, max_batch=8, backbone=True):
    from porl_amd.agent.fasternet import FasterNet
    from porl_amd.agent.por import POR
    from porl_amd.agent.sorl import SORL
    torch.manual_seed(seed)
    bb = FasterNet(3, 256, max_batch=max_batch, angle_bins=n_ang, dist_bins=n_dist, compute_dtype=dtype) if backbone else None
    args = SimpleNamespace(state_size=n_ang + 2, feature_dim=256, hidden_dim=64, n_hidden=2, layer_norm=False,
                           action_size=A, max_batch=max_batch)
    return (SORL if kind == "sorl" else POR)(args, max_steps=50, tau=0.9, alpha=3.0, device=DEV, backbone=bb)


def _optimizers(agent):
    return [agent.v_optimizer, getattr(agent, "policy_optimizer", None) or agent.goal_policy_optimizer]


def _assert_same_state(x, y):
    sx, sy = x.state_dict(), y.state_dict()
    assert list(sx) == list(sy)
    for k in sx:
        assert torch.equal(sx[k], sy[k]), k
    for ox, oy in zip(_optimizers(x), _optimizers(y)):
        assert ox.step_count == oy.step_count
        stx, sty = ox.state_dict()["state"], oy.state_dict()["state"]
        assert list(stx) == list(sty)
        for i in stx:
            for f in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(stx[i][f], sty[i][f]), (i, f)
    assert torch.equal(x._engine.stats[:3], y._engine.stats[:3])


def _tensor_step(agent, replay, idx, call="update"):
    """The tensor form on rows `idx`: gather, clone (the encoder clamps its input in place), split, update."""
    batch = replay.gather(idx).clone()
    s, r, s2, d, a = replay.split(batch)
    if hasattr(agent, "goal_policy"):
        return agent.por_residual_update(s, s2, r, d)
    return getattr(agent, call)(s, a, r, s2, d)


# ---- 1. the reference goldens through the row path -------------------------------------------------------------------------
def _golden_store(z, B, K, A):
    """The golden's K batches as one store, shuffled by a fixed permutation, and per batch the indices that restore it."""
    blocks = []
    for k in range(K):
        a = z[f"a{k}"] if f"a{k}" in z.files else np.zeros((B, A), dtype=np.float32)
        blocks.append(np.concatenate([z[f"s{k}"], z[f"r{k}"].reshape(B, 1), z[f"s2{k}"], z[f"d{k}"].reshape(B, 1),
                                      a.reshape(B, A)], axis=1).astype(np.float32))
    rows = np.concatenate(blocks)
    perm = np.random.default_rng(7).permutation(K * B)
    inv = np.argsort(perm)                                      # rows[perm][inv[j]] == rows[j]
    return rows[perm].copy(), [torch.from_numpy(inv[k * B:(k + 1) * B].copy()).to(DEV) for k in range(K)]


def test_sorl_golden_through_update_from_replay():
    """tests/test_fasternet_gpu.py:test_sorl_update_with_encoder_backbone_matches_reference_golden, rows read from a
    shuffled store by index instead of handed over as tensors: same seeds, same construction, same bounds."""
    from porl_amd.agent.fasternet import FasterNet
    from porl_amd.agent.sorl import SORL
    z, _ = load_golden("sorl_enc_b6")
    B, K, H, L, A, F = (int(v) for v in z["meta"])
    torch.manual_seed(int(z["seed_model"]))
    backbone = FasterNet(3, F, max_batch=B)
    args = SimpleNamespace(state_size=362, feature_dim=F, hidden_dim=H, n_hidden=L, layer_norm=False, action_size=A,
                           max_batch=B)
    agent = SORL(args, max_steps=50, tau=float(z["tau"]), alpha=float(z["alpha"]), device=DEV, backbone=backbone)
    sd = agent.state_dict()
    for k in z.files:
        if k.startswith("init."):
            assert np.array_equal(sd[k[5:]].cpu().numpy(), z[k]), k
    store, indices = _golden_store(z, B, K, A)
    replay = _replay(store, 362, A)
    torch.manual_seed(int(z["seed_fwd"]))
    for k in range(K):
        vl, gl = agent.update_from_replay(replay, B, indices=indices[k])
        print("losses", k, vl, gl, z["losses"][k])
        np.testing.assert_allclose([vl, gl], z["losses"][k], rtol=5e-5)
    sd = agent.state_dict()
    worst = 0.0
    for k in z.files:
        if not k.startswith("final."):
            continue
        got, ref = sd[k[6:]].cpu().numpy().astype(np.float64), z[k]
        if "num_batches" in k:
            assert int(got) == int(ref) == 2 * K
        elif "running_mean" in k:
            assert np.abs(got - ref).max() < 1e-5, k
        elif "running_var" in k:
            assert rel_err(got, ref) < 1e-5, k
        else:
            worst = max(worst, float(np.abs(got - ref).max()))
    print("worst", worst)
    assert worst < 2e-5, worst
    assert replay.draws == 0 and np.array_equal(replay.rows.cpu().numpy(), store)


def test_por_golden_through_update_from_replay():
    """test_por_with_encoder_backbone_matches_reference_golden through the row path (the goal policy regresses the raw
    362-wide next state, staged as the encoder's clamp would leave it)."""
    from porl_amd.agent.fasternet import FasterNet
    from porl_amd.agent.por import POR
    z, _ = load_golden("por_enc_b4")
    B, K, H, L, F = (int(v) for v in z["meta"])
    torch.manual_seed(int(z["seed_model"]))
    backbone = FasterNet(3, F, max_batch=B)
    args = SimpleNamespace(state_size=362, feature_dim=F, hidden_dim=H, n_hidden=L, layer_norm=False, action_size=2,
                           max_batch=B)
    agent = POR(args, max_steps=50, tau=float(z["tau"]), alpha=float(z["alpha"]), device=DEV, backbone=backbone)
    sd = agent.state_dict()
    for k in z.files:
        if k.startswith("init."):
            assert np.array_equal(sd[k[5:]].cpu().numpy(), z[k]), k
    store, indices = _golden_store(z, B, K, 2)
    replay = _replay(store, 362, 2)
    torch.manual_seed(int(z["seed_fwd"]))
    for k in range(K):
        vl, gl = agent.update_from_replay(replay, B, indices=indices[k])
        print("losses", k, vl, gl, z["losses"][k])
        np.testing.assert_allclose([vl, gl], z["losses"][k], rtol=5e-5)
    sd = agent.state_dict()
    worst = max(float(np.abs(sd[k[6:]].cpu().numpy().astype(np.float64) - z[k]).max()) for k in z.files if k.startswith("final."))
    print("worst", worst)
    assert worst < 2e-5, worst
    assert replay.draws == 0 and np.array_equal(replay.rows.cpu().numpy(), store)


# ---- 2. bit identity with the tensor path ----------------------------------------------------------------------------------------
N_STORE = 23
CASES = {
    #                 kind    n_ang n_dist A  B  dtype   steps  flags
    "sorl_fp32_84":  ("sorl", 84, 84, 3, 5, "fp32", 3, {}),                    # row width 177: odd stride
    "sorl_bf16_84":  ("sorl", 84, 84, 2, 8, "bf16", 3, {}),                    # B == max_batch
    "sorl_360_b1":   ("sorl", 360, 256, 2, 1, "fp32", 3, {}),
    "sorl_360_b6":   ("sorl", 360, 256, 2, 6, "fp32", 3, {}),
    "por_fp32_84":   ("por", 84, 84, 2, 4, "fp32", 3, {}),                     # clamp_target_gt8
    "dense_patch":   ("sorl", 84, 84, 2, 3, "fp32", 3, {"dense": True}),
    "two_phase":     ("sorl", 84, 84, 2, 4, "fp32", 3, {"phases": True}),
    "async":         ("sorl", 84, 84, 2, 4, "fp32", 3, {"async": True}),
    "eval_backbone": ("sorl", 84, 84, 2, 4, "fp32", 1, {"eval": True}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_update_from_replay_with_backbone_equals_the_tensor_path_bit_for_bit(case):
    from porl_amd import engine as E
    kind, n_ang, n_dist, A, B, dtype, steps, flags = CASES[case]
    S = n_ang + 2
    rows = _lidar_rows(N_STORE, n_ang, A, seed=n_ang + B)
    # the rows the three draws will take, from a third replay of the same seed; values > 8 go into the first row of each
    # draw: a beam of s, a beam of s', one goal coordinate of s'
    peek = _replay(rows, S, A, seed=5)
    drawn = [peek.sample_indices(B).cpu().tolist() for _ in range(steps)]
    for t, d in enumerate(drawn):
        assert len(set(d)) == B
        r = d[0]
        rows[r, 3 + t] = 9.0 + t
        rows[r, S + 1 + 10 + t] = 20.0
        rows[r, S + 1 + n_ang + (t % 2)] = 8.5
    try:
        if flags.get("dense"):
            E.tune_set("enc_dense_patch", 1)                     # engines copy the process defaults when they are created
        x, y = (_agent(kind, n_ang, n_dist, A, dtype) for _ in range(2))
    finally:
        E.tune_set("enc_dense_patch", 0)
    for ag in (x, y):
        ag.async_losses = bool(flags.get("async"))
        if flags.get("eval"):
            ag.backbone.eval()
    rx, ry = _replay(rows, S, A, seed=5), _replay(rows, S, A, seed=5)
    calls = ["vf_update", "policy_update", "vf_update"] if flags.get("phases") else ["update"] * steps
    torch.manual_seed(77)
    lx = []
    for c in calls:
        out = x.update_from_replay(rx, B) if c == "update" else getattr(x, c + "_from_replay")(rx, B)
        lx.append(None if x.async_losses else out)
    torch.manual_seed(77)
    ly = []
    for t, c in enumerate(calls):
        idx = ry.sample_indices(B)
        assert idx.cpu().tolist() == drawn[t]
        out = _tensor_step(y, ry, idx, c)
        ly.append(None if y.async_losses else out)
    x.flush()
    y.flush()
    assert lx == ly, (lx, ly)                                    # floats (tuples of floats), equal exactly
    _assert_same_state(x, y)
    nbt = [v for k, v in x.state_dict().items() if k.endswith("num_batches_tracked")]
    assert nbt and all(int(v) == (0 if flags.get("eval") else 2 * steps) for v in nbt)
    assert torch.equal(rx.rows, torch.from_numpy(rows).to(DEV))  # the store was only read ...
    assert float(rx.rows.max()) > 8.0                            # ... its planted values are still there
    assert rx.draws == steps and ry.draws == steps


# ---- 3. indices= without a backbone ----------------------------------------------------------------------------------------------
def _make_por(S, H, B, seed=0):
    from porl_amd.agent.por import POR
    torch.manual_seed(seed)
    args = SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=2, layer_norm=False, feature_dim=256, action_size=2,
                           max_batch=B)
    return POR(args, 1000, 0.9, 10.0, device=DEV)


def test_indices_without_a_backbone_equal_the_gathered_tensors():
    from porl_amd.util.synth import make_rows
    S, A, B, N = 60, 2, 7, 50
    rows = make_rows(N, S, A, seed=4)
    x, y = _make_por(S, 64, B), _make_por(S, 64, B)
    rx, ry = _replay(rows, S, A, seed=1), _replay(rows, S, A, seed=1)
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        idx = torch.randperm(N, generator=g)[:B].to(DEV)
        got = x.update_from_replay(rx, B, indices=idx)
        s, r, s2, d, _a = ry.split(ry.gather(idx))
        want = y.por_residual_update(s, s2, r, d)
        assert got == want
    _assert_same_state(x, y)
    assert rx.draws == 0 and torch.equal(rx.rows, ry.rows)


def test_the_device_draw_without_a_backbone_is_unchanged():
    """`update_from_replay(replay, B)` with no backbone and no indices: the one-kernel draw of porl_iql_load_batch_sampled,
    compared with the tensor form on the rows that kernel reports."""
    from porl_amd.util.synth import make_rows
    S, A, B, N = 60, 2, 7, 50
    rows = make_rows(N, S, A, seed=4)
    x, y = _make_por(S, 64, B), _make_por(S, 64, B)
    rx = _replay(rows, S, A, seed=1)
    rows_dev = torch.from_numpy(rows).to(DEV)
    for step in range(3):
        idx = torch.empty(B, dtype=torch.int64, device=DEV)
        x._engine.load_batch_sampled(rx.rows, B, rx.seed, rx.draws, A, False, idx_out=idx)      # peek at the draw
        got = x.update_from_replay(rx, B)
        batch = rows_dev[idx]
        want = y.por_residual_update(batch[:, :S], batch[:, S + 1:2 * S + 1], batch[:, S], batch[:, 2 * S + 1])
        assert got == want
    _assert_same_state(x, y)
    assert rx.draws == 3


# ---- 4. first and last row, named twice ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", [True, False])
def test_edge_rows_and_duplicates(backbone):
    from porl_amd.util.synth import make_rows
    B = 4
    if backbone:
        n_ang, A, N = 84, 2, N_STORE
        S = n_ang + 2
        rows = _lidar_rows(N, n_ang, A, seed=1)
        rows[N - 1, 2] = 11.0                                    # > 8 in the last row's s and in the first row's s'
        rows[0, S + 1 + 4] = 30.0
        x, y = (_agent("por", n_ang, 84, A) for _ in range(2))
    else:
        S, A, N = 60, 2, 50
        rows = make_rows(N, S, A, seed=6)
        x, y = _make_por(S, 64, B), _make_por(S, 64, B)
    rx, ry = _replay(rows, S, A), _replay(rows, S, A)
    idx = torch.tensor([N - 1, 0, N - 1, 0][:B], dtype=torch.int64, device=DEV)
    torch.manual_seed(5)
    got = x.update_from_replay(rx, B, indices=idx)
    torch.manual_seed(5)
    want = _tensor_step(y, ry, idx)
    assert got == want
    _assert_same_state(x, y)
    assert torch.equal(rx.rows, torch.from_numpy(rows).to(DEV)) and rx.draws == 0


# ---- 5. refusals launch nothing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", [True, False])
def test_refusals_leave_every_counter_alone(backbone):
    from porl_amd.util.synth import make_rows
    B = 4
    if backbone:
        n_ang, A, N = 84, 2, N_STORE
        S = n_ang + 2
        rows = _lidar_rows(N, n_ang, A, seed=2)
        agent = _agent("sorl", n_ang, 84, A, max_batch=B)
        sched = agent.lr_schedule
    else:
        S, A, N = 60, 2, 50
        rows = make_rows(N, S, A, seed=6)
        agent = _make_por(S, 64, B)
        sched = agent.goal_lr_schedule
    replay = _replay(rows, S, A)
    good = torch.arange(B, dtype=torch.int64, device=DEV)
    agent.update_from_replay(replay, B, indices=good)            # one accepted update first: counters are not all zero

    def counters():
        sd = agent.state_dict()
        return (replay.draws, [o.step_count for o in _optimizers(agent)], sched.last_epoch,
                [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")],
                {k: v.clone() for k, v in sd.items()})

    before = counters()
    narrow = _replay(make_rows(N, S - 1, A, seed=1), S - 1, A)
    with pytest.raises(ValueError, match=f"{S - 1}.*{S}"):
        agent.update_from_replay(narrow, B)
    with pytest.raises(ValueError):
        agent.update_from_replay(narrow, B, indices=good)
    with pytest.raises(RuntimeError):
        agent.update_from_replay(replay, B, indices=good.to(torch.int32))
    with pytest.raises(RuntimeError):
        agent.update_from_replay(replay, B, indices=good[:B - 1])
    with pytest.raises(RuntimeError):
        agent.update_from_replay(replay, B, indices=good.cpu())
    with pytest.raises(RuntimeError):
        agent.update_from_replay(replay, B + 1, indices=torch.arange(B + 1, dtype=torch.int64, device=DEV))   # > max_batch
    after = counters()
    assert before[:4] == after[:4]
    for k, v in before[4].items():
        assert torch.equal(v, after[4][k]), k
    assert narrow.draws == 0
    agent.update_from_replay(replay, B, indices=good)            # and the agent still works


# ---- 6. the data-parallel branch: forced one-rank exchange ------------------------------------------------------------------
def test_rows_path_through_the_forced_one_rank_exchange():
    """`update_from_replay` with a backbone on a one-rank RCCL group with the exchange forced on, in a process of its own
    (tests/helpers/enc_replay_world1.py): value_backward, exchange, Adam, policy phase (on the side stream under
    `async_losses`) behind the indexed load, bit-equal to the tensor form through the same exchange."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "helpers", "enc_replay_world1.py"), str(port)],
                       env=env, capture_output=True, text=True, timeout=300)
    skip = [ln for ln in r.stdout.splitlines() if ln.startswith("ENC_REPLAY_WORLD1_SKIP ")]
    if skip:
        pytest.skip(skip[0][len("ENC_REPLAY_WORLD1_SKIP "):])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ENC_REPLAY_WORLD1 ")]
    assert len(line) == 1
    out = json.loads(line[0][len("ENC_REPLAY_WORLD1 "):])
    assert out["backend"] == "nccl" and out["world"] == 1
    assert [c["async_losses"] for c in out["cases"]] == [False, True]
    for c in out["cases"]:
        assert c["bit_equal"] is True and c["losses_equal"] is True and c["store_untouched"] is True, c
        assert c["draws"] == 3 and c["steps"] == [3, 3], c
