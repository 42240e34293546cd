"""Run by tests/test_enc_replay_gpu.py in a process of its own: SORL with a FasterNet backbone on a process group of ONE
rank on backend "nccl" (= RCCL on ROCm) with the data-parallel exchange forced on (porl_amd.parallel.GradExchange
(force=True)), so that the one GPU of the test box takes the branch a multi-GPU job takes.  Two identically seeded agents,
both forced: one calls `update_from_replay` (rows encoded in place, indexed load), the other gathers the same draws and
calls `update`.  Both go through the same exchange, so every state tensor must agree bit for bit — with the losses read
back per update and with `async_losses` (policy phase pipelined on the side stream).  Prints one JSON line (or a SKIP
line where there is no usable backend)."""
import datetime
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)


def main():
    import numpy as np
    import torch
    import torch.distributed as dist
    from types import SimpleNamespace
    from porl_amd.agent.fasternet import FasterNet
    from porl_amd.agent.sorl import SORL
    from porl_amd.buffer.replay_buffer import PackedReplay

    if not dist.is_available() or not dist.is_nccl_available():
        print("ENC_REPLAY_WORLD1_SKIP torch.distributed has no nccl (RCCL) backend in this build", flush=True)
        return
    port = int(sys.argv[1])
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev,
                            timeout=datetime.timedelta(seconds=90))
    n_ang, A, B, N, U = 84, 2, 4, 23, 3
    S = n_ang + 2
    rng = np.random.default_rng(3)
    rows = np.empty((N, 2 * S + 2 + A), dtype=np.float32)
    for off in (0, S + 1):
        rows[:, off:off + n_ang] = rng.uniform(0.2, 3.9, size=(N, n_ang))
        rows[:, off + n_ang:off + S] = rng.uniform(-3, 3, size=(N, 2))
    rows[:, S] = rng.normal(size=N)
    rows[:, 2 * S + 1] = rng.uniform(size=N) < 0.2
    rows[:, 2 * S + 2:] = rng.uniform(-1, 1, size=(N, A))
    rows[::3, 5] = 9.0                                           # > 8: read as 0 by the rows path, zeroed in the copy by the other
    rows[1::3, S + 1 + 7] = 12.0

    def agent():
        torch.manual_seed(0)
        bb = FasterNet(3, 256, max_batch=8, angle_bins=n_ang, dist_bins=84)
        a = SORL(SimpleNamespace(state_size=S, feature_dim=256, hidden_dim=64, n_hidden=2, layer_norm=False, action_size=A,
                                 max_batch=8), 50, 0.9, 3.0, device=dev, backbone=bb)
        a._exchange.force = True
        return a

    out = {"backend": dist.get_backend(), "world": dist.get_world_size(), "cases": []}
    for async_losses in (False, True):
        x, y = agent(), agent()
        assert x._exchange.active and x._exchange.world_size == 1
        x.async_losses = y.async_losses = async_losses
        rx, ry = PackedReplay(rows, S, A, dev, seed=2), PackedReplay(rows, S, A, dev, seed=2)
        torch.manual_seed(11)
        lx = [x.update_from_replay(rx, B) for _ in range(U)]
        torch.manual_seed(11)
        ly = []
        for _ in range(U):
            s, r, s2, d, a = ry.split(ry.gather(ry.sample_indices(B)).clone())
            ly.append(y.update(s, a, r, s2, d))
        x.flush()
        y.flush()
        for o in (x.v_optimizer, x.policy_optimizer, y.v_optimizer, y.policy_optimizer):
            o.consolidate_state()
        sx, sy = x.state_dict(), y.state_dict()
        same = all(torch.equal(sx[k], sy[k]) for k in sx)
        for ox, oy in ((x.v_optimizer, y.v_optimizer), (x.policy_optimizer, y.policy_optimizer)):
            stx, sty = ox.state_dict()["state"], oy.state_dict()["state"]
            same = same and all(torch.equal(stx[i][f], sty[i][f]) for i in stx for f in ("exp_avg", "exp_avg_sq"))
        same = same and bool(torch.equal(x._engine.stats[:3], y._engine.stats[:3]))
        out["cases"].append(dict(async_losses=async_losses, bit_equal=bool(same),
                                 losses_equal=bool(async_losses or lx == ly), draws=rx.draws,
                                 store_untouched=bool(torch.equal(rx.rows.cpu(), torch.from_numpy(rows))),
                                 steps=[x.v_optimizer.step_count, x.policy_optimizer.step_count]))
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print("ENC_REPLAY_WORLD1 " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
