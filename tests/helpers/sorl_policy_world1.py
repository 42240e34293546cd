"""Run by tests/test_sorl_phases_gpu.py in a process of its own: SORL.policy_update on a process group of ONE rank on
backend "nccl" (= RCCL on ROCm) with the data-parallel exchange forced on (porl_amd.parallel.GradExchange(force=True)),
so that the one GPU of the test box takes the branch a multi-GPU job takes — forward half, backward, then
reduce-scatter + sharded Adam + all-gather ("reduce_scatter") or all-reduce + whole-group Adam ("all_reduce"), and the
statistics all-reduce.  A SUM over one rank changes no number, so from identical state every update must reproduce the
plain single-GPU policy-only step.  Prints one JSON line (or a SKIP line where there is no usable backend)."""
import datetime
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)


def main():
    import torch
    import torch.distributed as dist
    from types import SimpleNamespace
    from porl_amd.agent.sorl import SORL
    from porl_amd.util.synth import make_rows, split_rows

    if not dist.is_available() or not dist.is_nccl_available():
        print("SORL_POLICY_WORLD1_SKIP torch.distributed has no nccl (RCCL) backend in this build", flush=True)
        return
    port = int(sys.argv[1])
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev,
                            timeout=datetime.timedelta(seconds=90))
    out = {"backend": dist.get_backend(), "world": dist.get_world_size(), "cases": []}
    S, A, H, B, U = 60, 2, 256, 256, 3

    def agent(force):
        torch.manual_seed(0)
        a = SORL(SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=2, layer_norm=False, action_size=A, max_batch=B),
                 1000, 0.9, 3.0, device=dev)
        a._exchange.force = force
        return a

    rows = torch.from_numpy(make_rows((U + 2) * B, S, A, seed=9)).to(dev)
    batch = lambda k: split_rows(rows[k * B:(k + 1) * B], S, A)

    def pol_moments(a):
        a.policy_optimizer.consolidate_state()
        st = a.policy_optimizer.state_dict()["state"]
        return [st[i]["exp_avg"].clone() for i in sorted(st)]

    def value_state(a):
        a.v_optimizer.consolidate_state()
        e = a._engine
        return [t.clone() for t in (e.params_vf, e.params_tgt, e.adam_m_vf, e.adam_v_vf)] + [a.v_optimizer.step_count]

    for exchange in ("reduce_scatter", "all_reduce"):
        plain, forced = agent(False), agent(True)
        forced.grad_exchange = exchange
        assert forced._exchange.active and forced._exchange.world_size == 1 and not plain._exchange.active
        for k in range(2):                           # a value step and a joint step: moments and targets off their initial values
            s, r, sp, d, a = batch(k)
            if k == 0:
                plain.vf_update(s, a, r, sp, d)
            else:
                plain.update(s, a, r, sp, d)
        beta1 = plain.policy_optimizer.param_groups[0]["betas"][0]
        per, frozen_ok = [], True
        for u in range(U):
            forced.load_state_dict(plain.state_dict())
            forced.v_optimizer.load_state_dict(plain.v_optimizer.state_dict())
            forced.policy_optimizer.load_state_dict(plain.policy_optimizer.state_dict())
            forced.lr_schedule.load_state_dict(plain.lr_schedule.state_dict())
            forced._engine.stats.copy_(plain._engine.stats)
            m_old = pol_moments(plain)
            frozen = value_state(forced)
            s, r, sp, d, a = batch(2 + u)
            lp = plain.policy_update(s, a, r, sp, d)
            lf = forced.policy_update(s, a, r, sp, d)
            m_p, m_f = pol_moments(plain), pol_moments(forced)
            grad_err = 0.0
            for old, mp, mf in zip(m_old, m_p, m_f):
                g = mp - beta1 * old                     # (1 - beta1) * g of the plain update
                grad_err = max(grad_err, float((mf - mp).abs().max()) / max(1e-30, float(g.abs().max())))
            sd_p, sd_f = plain.state_dict(), forced.state_dict()
            now = value_state(forced)
            frozen_ok = frozen_ok and now[-1] == frozen[-1] and all(torch.equal(x, y) for x, y in zip(now[:-1], frozen[:-1]))
            frozen_ok = frozen_ok and bool(forced._engine.stats[0] == plain._engine.stats[0])
            per.append(dict(max_rel_loss_err=abs(lf / lp - 1), max_rel_grad_err=grad_err,
                            max_abs_param_err=max(float((sd_f[k] - sd_p[k]).abs().max()) for k in sd_p)))
        assert forced.policy_optimizer.step_count == plain.policy_optimizer.step_count
        out["cases"].append(dict(exchange=exchange, per_update=per, value_state_unchanged=frozen_ok,
                                 sharded=bool(forced.policy_optimizer.sharded)))
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print("SORL_POLICY_WORLD1 " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
