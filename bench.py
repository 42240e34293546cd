#!/usr/bin/env python3
"""Headline benchmark: POR gradient-steps/sec (BASELINE.json metric) on N MI355X of one node.

    python bench.py --gpus 1 --steps 200 --warmup 20
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one full POR update (agent/por.py:73-112 of the reference) INCLUDING minibatch
acquisition: draw B distinct rows of the device-resident replay shard, gather them, run value step +
EMA + policy step.  Workload at N=1 is BASELINE config 2 (S=60, A=2, H=1024, L=2, B=1024, 1 M-row
buffer, fp32); at N>1 every rank keeps its own 1.25 M-row shard (N=8 -> the 10 M-row buffer of config 4)
and draws B=1024 local rows — weak scaling, gradients exchanged with RCCL.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the
line: nothing else.  At N>1 the line carries
  dp           : which data-parallel modes ran, which one `value` is from, what failed
With --full an N=1 run goes on after the timed steps and adds (each --no-* option still drops its part)
  sustained_1000_updates_per_sec : the same loop again for 5 x 1 000 updates, median
  roofline     : dominant launch (the 4-net hidden-layer fp32-MFMA grouped GEMM) timed with HIP events on its
                 launch stream in a second, instrumented pass
  secondary    : BASELINE configs 3 and 5, POR at the class-default width and the headline in the reference's
                 synchronous calling convention — each its own short timed loop, none of them `value`
  cpu_baseline : eager PyTorch-CPU / the numpy oracle (oracle/) timed on the host cores on a bounded sample of the
                 same workload
and `--workload cql|sorl_enc` adds its instrumented roofline pass and its CPU baseline.

N > 1.  Every GPU process is the CHILD of a supervisor that makes no GPU call: under
torch.distributed.run each launched rank supervises its own child, for the bare `python bench.py --gpus N` one
parent starts and supervises all N.  The child times the data-parallel modes from the most conservative to the
most aggressive — SUM all-reduce on one stream; reduce-scatter -> sharded Adam -> all-gather on one stream; the same
pipelined over two streams with one RCCL communicator; with a communicator of its own for the policy group — and
reports after each.  A mode that dies or hangs (process-group timeout, supervisor deadline: the exact child PIDs are
killed) costs only itself: the line is built from the modes that finished, `value` = the best of them, and
`dp.failed` names the rest.  No rank is ever re-executed in place.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0     # MI355X_MICROARCH.md: dense bf16
PEAK_HBM_GBS = 8000.0              # MI355X_MICROARCH.md: HBM3E
S, A, H, L, B = 60, 2, 1024, 2, 1024

DP_MODES = ("allreduce_1stream", "reduce_scatter_1stream", "reduce_scatter_pipelined_1comm", "reduce_scatter_pipelined_2comm")


DUMP_BUDGET_BYTES = 63_000_000     # --dump-outputs: array data of all files (the .npy headers stay well inside 64 MB)


def dump_outputs(out_dir, arrays):
    """--dump-outputs: write what the timed path computed in its last step as <out_dir>/<name>.npy, float32 kept,
    anything else as float64.  When the whole set exceeds the budget, each array larger than its share is replaced
    by a fixed, seeded sample of its elements (flat, indices sorted; the seed is keyed by the name), so that two builds
    run with the same arguments can be compared element for element."""
    import zlib
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrs = {}
    for name, v in arrays.items():
        x = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        arrs[name] = x.astype(np.float32 if x.dtype == np.float32 else np.float64, copy=False)
    left, total = DUMP_BUDGET_BYTES, 0
    order = sorted(arrs, key=lambda k: (arrs[k].nbytes, k))
    for i, name in enumerate(order):
        x = arrs[name]
        share = left // (len(order) - i)
        if x.nbytes > share:
            rng = np.random.default_rng(zlib.crc32(name.encode()))
            x = x.ravel()[np.sort(rng.choice(x.size, share // x.itemsize, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), x)
        left -= x.nbytes
        total += x.nbytes
    sys.stderr.write(f"[bench] {len(order)} output arrays ({total / 1e6:.1f} MB) written to {out_dir}\n")


def por_flops_per_sample(h=None):
    """14 440 448 MAC per sample at H=1024."""
    h = h or H
    mac_v = S * h + h * h + h
    mac_p = S * h + h * h + h * S
    fwd = 6 * mac_v + mac_p
    bwd = 2 * (mac_v + h * h + h) + (mac_p + h * h + h * S)
    return 2 * (fwd + bwd)


# =====================================================================================================================
# CPU baselines (rank 0, N=1, --full only).  oracle/ is test infrastructure: it is imported HERE and nowhere in the timed GPU path.
# =====================================================================================================================
def cpu_baseline(budget_s=12.0):
    """CPU steps/s on the host, same shapes, bounded by wall time: the stronger of (a) eager PyTorch-CPU (MKL,
    autograd, torch.optim.Adam — how the reference itself runs; oracle/torch_cpu.py) and (b) the numpy oracle
    (oracle/por_oracle.py), each with its thread count tuned by a few trial steps so that oversubscription does not
    handicap it.  Both are this repository's restatements ("port"); the reference's files never travel to this box."""
    import numpy as np
    import torch
    from oracle.por_oracle import PorOracle
    from oracle.torch_cpu import PorTorchCpu
    from porl_amd.util.init import build_por_state_dict
    from porl_amd.util.synth import make_rows, split_rows
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        max_threads = max([p.get("num_threads", 1) for p in threadpool_info()] or [1])
    except Exception:
        threadpool_limits, max_threads = None, os.cpu_count() or 1
    sd = build_por_state_dict(S, H, L, seed=0)
    rows = make_rows(8 * B, S, A, seed=0)
    batches = [split_rows(rows[k * B:(k + 1) * B], S, A)[:4] for k in range(8)]

    def run(step, budget):
        step(0)                                                  # warm-up (thread pools, page faults)
        n, t0 = 0, time.perf_counter()
        while True:
            step(n)
            n += 1
            el = time.perf_counter() - t0
            if el >= budget and n >= 3:
                return n, el

    # (a) eager PyTorch on the CPU
    tb = [tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in (s, sp, r, d)) for s, r, sp, d in batches]
    ncpu = os.cpu_count() or 1
    best_tt, best_rate = torch.get_num_threads(), 0.0
    for tt in sorted({t for t in (8, 16, 32, 64, ncpu) if t <= ncpu}):
        torch.set_num_threads(tt)
        m = PorTorchCpu(sd, S, H, L)
        n, el = run(lambda i: m.update(*tb[i % 8]), 0.6)
        if n / el > best_rate:
            best_tt, best_rate = tt, n / el
    torch.set_num_threads(best_tt)
    m = PorTorchCpu(sd, S, H, L)
    nt, elt = run(lambda i: m.update(*tb[i % 8]), budget_s / 2)
    cand = [dict(value=nt / elt, cores=int(best_tt), impl="eager PyTorch-CPU (oracle/torch_cpu.py)", n=nt, el=elt)]
    # (b) numpy oracle
    o = PorOracle(build_por_state_dict(S, H, L, seed=0), S, H, L)
    nb = [(s, sp, r, d) for s, r, sp, d in batches]
    best_t, best_rate = max_threads, 0.0
    if threadpool_limits is not None:
        for t in sorted({t for t in (8, 16, 32, 64, max_threads) if t <= max_threads}):
            with threadpool_limits(limits=t):
                n, el = run(lambda i: o.por_residual_update(*nb[i % 8]), 0.4)
            if n / el > best_rate:
                best_t, best_rate = t, n / el
    ctx = threadpool_limits(limits=best_t) if threadpool_limits is not None else None
    try:
        nn_, eln = run(lambda i: o.por_residual_update(*nb[i % 8]), budget_s / 2)
    finally:
        if ctx is not None and hasattr(ctx, "restore_original_limits"):
            ctx.restore_original_limits()
    cand.append(dict(value=nn_ / eln, cores=int(best_t), impl="numpy oracle (oracle/por_oracle.py)", n=nn_, el=eln))
    best = max(cand, key=lambda c: c["value"])
    other = min(cand, key=lambda c: c["value"])
    return dict(value=best["value"], unit="gradient-steps/sec", cores=best["cores"], kind="port",
                sample=f"{best['n']} POR updates (B={B}, H={H}, S={S}) of {best['impl']}, {best['cores']} threads (tuned), "
                       f"in {best['el']:.1f} s; the other port, {other['impl']} on {other['cores']} threads: "
                       f"{other['value']:.1f} steps/s")


# =====================================================================================================================
# Secondary workloads: BASELINE configs 3 (CQL) and 5 (SORL + costmap encoder).  `--workload cql|sorl_enc` prints their
# own line; a --full run of the headline folds a short form of each into `secondary`.
# =====================================================================================================================
def measure_cql(steps, warmup, with_cpu=True, dump_dir=None, with_roofline=True):
    """BASELINE config 3: CQL(H) learn() at B=4096, S=60, A=10, Q-net 64-128-64, 100 k-row buffer resident on the
    device, rows drawn by the step kernel itself.  dump_dir: the last timed step's losses and networks (dump_outputs).
    with_roofline: the instrumented second pass behind `roofline`."""
    import numpy as np
    import torch
    from porl_amd.train.cql_trainer import CQLTrainer
    from porl_amd.util.synth import make_discrete_transitions
    from porl_amd import engine as E
    _apply_tuning_env(E)
    dev = torch.device("cuda", torch.cuda.current_device())
    Sq, Aq, Bq, Nq = 60, 10, 4096, 100_000
    torch.manual_seed(0)
    t = CQLTrainer(state_size=Sq, action_size=Aq, gamma=0.99, device=dev, batch_size=Bq)
    st, ac, rw, ns, dn = make_discrete_transitions(Nq, Sq, Aq, seed=0)
    rb = t.replay_buffer
    rb.states[:Nq], rb.actions[:Nq], rb.rewards[:Nq], rb.next_states[:Nq], rb.dones[:Nq] = st, ac, rw, ns, dn
    rb.size, rb.position = Nq, 0
    t.async_losses = True
    for i in range(warmup):
        t.learn_device_sampled()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        t.learn_device_sampled()
        if i % 10 == 0:
            t.sync_target()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    if not np.isfinite(t._engine.stats[:3].cpu().numpy()).all():
        raise RuntimeError("non-finite CQL loss")
    if dump_dir:
        # [loss, td_loss, cql_penalty] of the last timed step, then the networks it left behind
        arrays = {"losses": t._engine.stats[:3]}
        for prefix, net in (("q_network.", t.q_network), ("target_network.", t.target_network)):
            arrays.update({prefix + k: v for k, v in net.state_dict().items()})
        dump_outputs(dump_dir, arrays)
    prof = []
    if with_roofline:
        # instrumented second pass: HIP events around the step kernel on its launch stream
        psteps = max(steps, 50)
        E.prof_enable(True)
        for i in range(psteps):
            t.learn_device_sampled()
        prof = E.prof_read()
        E.prof_enable(False)
    roof = None
    dom = [p for p in prof if p["name"].startswith(("qnet_fused", "qnet_resident")) and p["launches"]]
    if dom:
        d0 = max(dom, key=lambda p: p["total_ms"])
        # the step is HBM/latency-bound; algorithmic bytes = gathered rows + parameters/Adam state
        n_par = sum(p.numel() for p in t.q_network.parameters())
        alg_bytes = Bq * (2 * Sq + 3) * 4 + Bq * 8 + n_par * 28
        avg_us = 1e3 * d0["total_ms"] / d0["launches"]
        ach = alg_bytes / (avg_us * 1e-6) / 1e9
        tf = 2.0 * 138368 * Bq / (avg_us * 1e-6) / 1e12
        roof = dict(bound="hbm", kernel=d0["name"], achieved=ach, peak=PEAK_HBM_GBS, unit="GB/s", frac=ach / PEAK_HBM_GBS,
                    traffic=_committed_traffic("r03_counters_cql.json", d0["name"]) or _committed_traffic("r02_counters_cql.json", d0["name"]),
                    avg_launch_us=avg_us, launches=d0["launches"], algorithmic_bytes_per_launch=alg_bytes,
                    # the other roof (138 368 MAC per sample = 3 forward + 2 backward passes of the
                    # 20 864-MAC network)
                    mfma_tflops=tf, mfma_frac=tf / PEAK_FP32_MFMA_TFLOPS,
                    all_kernels_us_per_step={p["name"]: round(1e3 * p["total_ms"] / psteps, 2) for p in prof if p["launches"]})
    out = {"metric": "gradient-steps/sec (CQL learn, batch=4096)", "value": steps / el,
           "unit": "gradient-steps/sec", "n_gpus": 1, "steps": steps, "warmup": warmup,
           "ms_per_step": 1e3 * el / steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": "CQL S=60 A=10 B=4096 Q-net 64-128-64, 100k-row device-resident buffer, indices drawn "
                                  "and rows gathered on the device"}}
    if roof:
        out["roofline"] = roof
    if with_cpu:
        # CPU baseline: eager PyTorch-CPU restatement (oracle/torch_cpu.py: autograd + torch.optim.Adam, like the reference
        # runs) incl. numpy's O(N) sampling as buffer/replay_buffer.py:64 does it, threads tuned; the numpy oracle beside it
        from oracle.por_oracle import CqlOracle
        from oracle.torch_cpu import CqlTorchCpu
        qsd = {k: v.detach().cpu().numpy() for k, v in t.q_network.state_dict().items()}
        rng = np.random.default_rng(0)
        tst, tac, trw, tns, tdn = (torch.from_numpy(x) for x in (st, ac, rw, ns, dn))

        def torch_rate(budget, threads):
            torch.set_num_threads(threads)
            m = CqlTorchCpu(qsd, Aq)
            n, c0 = 0, time.perf_counter()
            while time.perf_counter() - c0 < budget:
                idx = torch.from_numpy(rng.choice(Nq, Bq, replace=False))
                m.learn(tst[idx], tac[idx], trw[idx], tns[idx], tdn[idx])
                n += 1
            return n / (time.perf_counter() - c0), n

        ncpu = os.cpu_count() or 1
        best_tt = max(sorted({x for x in (1, 4, 8, 16, 32) if x <= ncpu}), key=lambda x: torch_rate(0.5, x)[0])
        cpu, n = torch_rate(4.0, best_tt)
        o = CqlOracle(qsd, Aq)
        n2, c0 = 0, time.perf_counter()
        while time.perf_counter() - c0 < 2.0:
            idx = rng.choice(Nq, Bq, replace=False)
            o.learn(st[idx], ac[idx], rw[idx], ns[idx], dn[idx])
            n2 += 1
        cpu_np = n2 / (time.perf_counter() - c0)
        out["cpu_baseline"] = {"value": cpu, "unit": "gradient-steps/sec", "kind": "port", "cores": int(best_tt),
                               "sample": f"{n} learn() steps of the eager PyTorch-CPU restatement (oracle/torch_cpu.py) incl. numpy "
                                         f"sampling, {best_tt} threads (tuned) in 4 s; numpy oracle: {cpu_np:.1f} steps/s"}
    return out


def measure_sorl_enc(steps, warmup, batch=512, angle_bins=360, dist_bins=256, enc_dtype="fp32", with_cpu=True,
                     dump_dir=None, with_roofline=True):
    """BASELINE config 5: SORL.update with the FasterNet costmap encoder as backbone, S = angle_bins + 2 (beams + goal),
    feature_dim=256, H=512.  One step = encode s, encode s' (train-mode BatchNorm, DropPath), value + policy update.
    fp32 on the reference's 360x256 image is the parity configuration; 84x84 / bf16 are BASELINE's wording.
    dump_dir: the last timed step's losses and the agent's state (dump_outputs).  with_roofline: the instrumented
    second pass behind `roofline`."""
    import numpy as np
    import torch
    from types import SimpleNamespace
    from porl_amd.agent.fasternet import FasterNet
    from porl_amd.agent.sorl import SORL
    from porl_amd import engine as E
    _apply_tuning_env(E)
    dev = torch.device("cuda", torch.cuda.current_device())
    Bq, F, Hq, Aq = batch, 256, 512, 2
    torch.manual_seed(0)
    n_ang, n_dist = angle_bins, dist_bins
    backbone = FasterNet(3, F, max_batch=Bq, angle_bins=n_ang, dist_bins=n_dist, compute_dtype=enc_dtype)
    args = SimpleNamespace(state_size=n_ang + 2, feature_dim=F, hidden_dim=Hq, n_hidden=2, layer_norm=False, action_size=Aq,
                           max_batch=Bq)
    agent = SORL(args, max_steps=1000, tau=0.9, alpha=3.0, device=dev, backbone=backbone)
    agent.async_losses = True
    rng = np.random.default_rng(0)
    nb = 4
    st = np.empty((nb, 2, Bq, n_ang + 2), dtype=np.float32)
    st[..., :n_ang] = rng.uniform(0.15, 3.9, size=(nb, 2, Bq, n_ang))
    st[..., n_ang:] = rng.uniform(-3, 3, size=(nb, 2, Bq, 2))
    st = torch.from_numpy(st).to(dev)
    act = torch.from_numpy(rng.uniform(-1, 1, size=(nb, Bq, Aq)).astype(np.float32)).to(dev)
    rew = torch.from_numpy(rng.normal(size=(nb, Bq)).astype(np.float32)).to(dev)
    done = torch.from_numpy((rng.uniform(size=(nb, Bq)) < 0.1).astype(np.float32)).to(dev)

    def one_step(i):
        k = i % nb
        agent.update(st[k, 0], act[k], rew[k], st[k, 1], done[k])

    import gc
    gc.collect()
    gc.disable()                                   # (a collector pause inside a 50 ms window showed up as 614 instead of 930 updates/s)
    try:
        for i in range(warmup):
            one_step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            one_step(i)
        agent.flush()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
    finally:
        gc.enable()
    losses = agent._engine.stats[:2].cpu().numpy()
    if not np.isfinite(losses).all():
        raise RuntimeError("non-finite loss in the SORL + encoder run")
    if dump_dir:
        # [v_loss, g_loss, min_nll] of the last timed step, then parameters and BatchNorm statistics (encoder included)
        dump_outputs(dump_dir, {"losses": agent._engine.stats[:3], **agent.state_dict()})
    enc_flops = 2 * 2 * Bq * 0.86e9 * (n_ang * n_dist) / (360.0 * 256.0)
    roof = None
    if with_roofline:
        psteps = min(steps, 10)
        E.prof_enable(True)
        for i in range(psteps):
            one_step(i)
        prof = E.prof_read()
        E.prof_enable(False)
        split = {p["name"]: round(p["total_ms"] / psteps, 4) for p in prof if p["launches"]}
        gemms = [p for p in prof if p["name"].split(":")[-1].startswith(("gemm_f32_kernel", "gemm_bf16_kernel", "enc_")) and p["launches"]
                 and p["flops"] > 0]
        dom = max(gemms, key=lambda p: p["total_ms"])
        ach = dom["flops"] / (dom["total_ms"] * 1e-3) / 1e12
        hbm = dom["bytes"] / (dom["total_ms"] * 1e-3) / 1e9
        peak_tf = PEAK_FP32_MFMA_TFLOPS if enc_dtype == "fp32" else PEAK_BF16_MFMA_TFLOPS
        roof = dict(kernel=dom["name"], launches=dom["launches"], avg_launch_us=1e3 * dom["total_ms"] / dom["launches"], traffic=None,
                    mfma_tflops=ach, mfma_frac=ach / peak_tf, hbm_gbs=hbm, hbm_frac=hbm / PEAK_HBM_GBS,
                    all_kernels_ms_per_step=split)
        if enc_dtype == "fp32":
            roof.update(bound="mfma", achieved=ach, peak=peak_tf, unit="TFLOP/s", frac=ach / peak_tf)
        else:
            roof.update(bound="hbm", achieved=hbm, peak=PEAK_HBM_GBS, unit="GB/s", frac=hbm / PEAK_HBM_GBS)
    out = {"metric": "gradient-steps/sec (SORL update + FasterNet encoder, batch=%d)" % Bq, "value": steps / el,
           "unit": "gradient-steps/sec", "n_gpus": 1, "steps": steps, "warmup": warmup,
           "ms_per_step": 1e3 * el / steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32" if enc_dtype == "fp32" else "bf16 (encoder products and activations between them; f32 accumulate, f32 heads)",
           "data": "synthetic",
           "config": {"workload": f"SORL S={n_ang + 2} F={F} H={Hq} B={Bq} + FasterNet(3,{F}) encoder on {n_ang}x{n_dist} costmaps, "
                                  "2 encoder forwards (train-mode BN, DropPath) + value/policy update per step"},
           "algorithmic_tflops": enc_flops * steps / el / 1e12}
    if roof:
        out["roofline"] = roof
    if with_cpu:
        sys.path.insert(0, os.path.join(REPO, "oracle"))
        import fasternet_oracle as FO
        sd = {k: v.cpu().numpy() for k, v in backbone.state_dict().items()}
        stats = {k: v.copy() for k, v in sd.items() if "running" in k}
        bs = 8
        x = st[0, 0, :bs].cpu().numpy()
        c0 = time.perf_counter()
        FO.forward(sd, stats, x.copy(), True, np.ones((3, bs), np.float32), dtype=np.float32, angle_bins=n_ang, dist_bins=n_dist)
        FO.forward(sd, stats, x.copy(), True, np.ones((3, bs), np.float32), dtype=np.float32, angle_bins=n_ang, dist_bins=n_dist)
        dt = time.perf_counter() - c0
        out["cpu_baseline"] = {"value": (bs / Bq) / dt, "unit": "gradient-steps/sec", "kind": "port", "cores": os.cpu_count(),
                               "sample": f"2 encoder forwards of oracle/fasternet_oracle.py (numpy fp32) on {bs} of the "
                                         f"{Bq} samples in {dt:.1f} s, scaled by {bs}/{Bq}; heads' update excluded (<1 %)"}
    return out


def _committed_traffic(fname, kernel):
    """HBM bytes per launch from a committed rocprofv3 --pmc pass (profiles/), or None."""
    try:
        tj = json.load(open(os.path.join(REPO, "profiles", fname)))
        k = tj["kernels"]
        import re
        norm = lambda n: re.sub(r"\d", "", n.split("@")[0].split("<")[0].split(":")[-1])     # qnet_fused2_kernel<32>@128 -> qnet_fused_kernel
        for name, v in k.items():
            if name == kernel or norm(name) == norm(kernel):
                return v.get("hbm_bytes_per_launch")
    except Exception:
        pass
    return None


def _brief(o, keys=("value", "ms_per_step", "steps", "warmup", "dtype")):
    d = {k: o[k] for k in keys if k in o}
    d["workload"] = o["config"]["workload"]
    r = o.get("roofline")
    if r:
        d["dominant_kernel"] = {k: r[k] for k in ("kernel", "avg_launch_us", "bound", "frac", "mfma_frac", "hbm_frac", "traffic")
                                if k in r and r[k] is not None}
        if "hbm_frac" not in d["dominant_kernel"] and r.get("bound") == "hbm":
            d["dominant_kernel"]["hbm_frac"] = r["frac"]
    return d


# =====================================================================================================================
# Supervisor: a process that makes no GPU call, starts the rank process(es), follows their progress markers and builds
# the line from whatever finished.
# =====================================================================================================================
def supervise(n_children, launched_by_torchrun):
    import socket
    import subprocess
    import threading
    setup_deadline = float(os.environ.get("PORL_BENCH_SETUP_DEADLINE_S", "330"))     # start -> first mode finished
    mode_deadline = float(os.environ.get("PORL_BENCH_MODE_DEADLINE_S", "100"))       # between two progress markers
    base_env = dict(os.environ, PORL_BENCH_CHILD="1", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONUNBUFFERED="1")
    procs = []
    if launched_by_torchrun:
        my_rank = int(os.environ.get("RANK", "0"))
        envs = [base_env]
    else:
        my_rank = 0
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
        sock.close()
        envs = [dict(base_env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n_children), LOCAL_WORLD_SIZE=str(n_children),
                     MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)) for r in range(n_children)]
    for env in envs:
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE, text=True, bufsize=1))
    state = dict(last=time.monotonic(), modes=[], final=None, markers=[0] * len(procs))
    lock = threading.Lock()

    def reader(i, p):
        for ln in p.stdout:
            ln = ln.rstrip("\n")
            with lock:
                if ln.startswith("PORL_MODE_DONE "):
                    state["markers"][i] += 1
                    state["last"] = time.monotonic()
                elif ln.startswith("PORL_MODE "):
                    state["modes"].append(json.loads(ln[len("PORL_MODE "):]))
                elif ln.startswith("PORL_FINAL "):
                    state["final"] = ln[len("PORL_FINAL "):]
                    state["last"] = time.monotonic()
                elif ln.strip():
                    sys.stderr.write(f"[rank-child {i}] {ln}\n")

    threads = [threading.Thread(target=reader, args=(i, p), daemon=True) for i, p in enumerate(procs)]
    for t in threads:
        t.start()
    t_start = time.monotonic()
    note = None

    def kill_all(why):
        nonlocal note
        alive = [i for i, p in enumerate(procs) if p.poll() is None]
        note = f"{why}; killed child processes {[procs[i].pid for i in alive]} (children {alive} were alive)"
        sys.stderr.write("[bench supervisor] " + note + "\n")
        for i in alive:
            procs[i].kill()                                   # exactly the PIDs started above

    while any(p.poll() is None for p in procs):
        time.sleep(0.2)
        now = time.monotonic()
        with lock:
            started = min(state["markers"]) > 0
            idle = now - state["last"]
            done = state["final"] is not None
        bad = [i for i, p in enumerate(procs) if p.poll() not in (None, 0)]
        if bad:                                               # a dead rank leaves the others in a collective
            time.sleep(3.0)                                   # (let them fail by themselves first: clearer messages)
            kill_all(f"child {bad} exited with code {[procs[i].returncode for i in bad]}")
            break
        if done and idle > 30.0:
            kill_all("result printed but the children did not exit within 30 s")
            break
        if not done and (idle > mode_deadline if started else now - t_start > setup_deadline):
            kill_all(f"no progress marker for {idle:.0f} s" if started else f"no mode finished within {setup_deadline:.0f} s of start")
            break
    for p in procs:
        try:
            p.wait(timeout=15)
        except Exception:
            pass
    for t in threads:
        t.join(timeout=5)
    codes = [p.returncode for p in procs]
    with lock:
        final, modes, markers = state["final"], list(state["modes"]), list(state["markers"])
    if my_rank != 0:
        # under torchrun a non-zero exit of ANY worker tears the job down: this rank did its part if one mode finished
        raise SystemExit(0 if markers and min(markers) > 0 else 1)
    if final is not None:
        out = json.loads(final)
        if note:
            out.setdefault("dp", {})["note"] = note
    elif modes:
        ok = [m for m in modes if m.get("ok")]
        if not ok:
            raise SystemExit(f"no data-parallel mode finished ({note}); rank exit codes {codes}")
        out = dict(max(ok, key=lambda m: m["value"])["line"])
        ran = {m["mode"] for m in modes}
        wanted = [m for m in (os.environ.get("PORL_BENCH_MODES") or ",".join(DP_MODES)).split(",") if m]
        out["dp"].update(modes=[{k: v for k, v in m.items() if k != "line"} for m in modes],
                         failed=[m for m in wanted if m not in ran] + [m["mode"] for m in modes if not m.get("ok")],
                         note=(note or "") + f"; rank exit codes {codes}; line built by the supervisor from the modes that finished")
    else:
        raise SystemExit(f"no result from the rank processes ({note}); exit codes {codes}")
    print(json.dumps(out), flush=True)
    raise SystemExit(0)


# =====================================================================================================================
# The GPU process
# =====================================================================================================================
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="por", choices=["por", "cql", "sorl_enc"])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rows-per-gpu", type=int, default=0)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--hidden", type=int, default=0,
                    help="por: hidden width other than the headline's 1024 (e.g. 256, the reference's class default, "
                         "value_functions.py:32); with --batch for the small-network figures of DESIGN.md §7")
    ap.add_argument("--angle-bins", type=int, default=360, help="sorl_enc: costmap rows (360 = the reference's image)")
    ap.add_argument("--dist-bins", type=int, default=256, help="sorl_enc: costmap columns")
    ap.add_argument("--enc-dtype", default="fp32", choices=["fp32", "bf16", "bf16_operands"],
                    help="sorl_enc: operand type of the encoder's 1x1 / merge convolutions (fp32 = reference parity)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what the headline does not need: the sustained rate, the "
                         "instrumented roofline pass, the `secondary` workloads and the CPU baseline (N=1); the roofline "
                         "pass and the CPU baseline of --workload cql|sorl_enc")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="--full without the POR roofline pass")
    ap.add_argument("--no-secondary", action="store_true",
                    help="--full without the `secondary` object (configs 3 / 5, H=256, sync mode)")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="issue every update back to back on one stream (profiling: kernels never overlap)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (losses, parameters) as DIR/<name>.npy; "
                         "the inputs are seeded, so two builds run with the same arguments compare output for output")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.workload == "cql":
        print(json.dumps(measure_cql(a.steps, a.warmup, a.full and not a.no_cpu_baseline, a.dump_outputs,
                                     with_roofline=a.full)), flush=True)
        return
    if a.workload == "sorl_enc":
        print(json.dumps(measure_sorl_enc(a.steps, a.warmup, a.batch or 512, a.angle_bins, a.dist_bins, a.enc_dtype,
                                          a.full and not a.no_cpu_baseline, a.dump_outputs, with_roofline=a.full)),
              flush=True)
        return
    global H, B
    if a.hidden:
        H = a.hidden                        # not the headline configuration: config.workload says so
    if a.batch:
        B = a.batch
    force_dp = os.environ.get("PORL_BENCH_FORCE_DP") == "1"        # one rank, RCCL collectives really issued (tests)
    if a.dump_outputs and (a.gpus > 1 or force_dp):
        ap.error("--dump-outputs needs a single-process run (--gpus 1): the data-parallel run times several modes")
    if (a.gpus > 1 or force_dp) and os.environ.get("PORL_BENCH_CHILD") != "1":
        # this process never touches a GPU: it starts the rank process(es) and follows them
        return supervise(a.gpus, launched_by_torchrun="WORLD_SIZE" in os.environ and a.gpus > 1)
    por_rank(a, force_dp)


def por_rank(a, force_dp):
    import datetime
    import numpy as np
    import torch
    import torch.distributed as dist
    from types import SimpleNamespace

    world = int(os.environ.get("WORLD_SIZE", "1")) if a.gpus > 1 else 1
    rank = int(os.environ.get("RANK", "0")) if a.gpus > 1 else 0
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if a.gpus > 1 else 0
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dp = world > 1 or force_dp
    # PORL_BENCH_BACKEND=gloo rehearses the N>1 code path with several ranks on ONE GPU (no RCCL, no timing claim)
    backend = os.environ.get("PORL_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if dp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
            os.environ["PORL_DP_FORCE"] = "1"                  # parallel.GradExchange: active in a one-rank group
        # a collective that does not complete within this time aborts the process (the supervisor then falls back on
        # the modes that finished) instead of hanging until the driver's limit
        pg_timeout = datetime.timedelta(seconds=float(os.environ.get("PORL_BENCH_PG_TIMEOUT_S", "90")))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=pg_timeout)
        else:
            dist.init_process_group(backend, timeout=pg_timeout)

    from porl_amd.agent.por import POR
    from porl_amd.buffer.replay_buffer import PackedReplay
    from porl_amd.util.synth import make_rows
    from porl_amd import engine as E

    rows_per_gpu = a.rows_per_gpu or (1_000_000 if world == 1 else 1_250_000)
    # every rank generates only its own shard (same generator family, rank-keyed seed)
    shard = make_rows(rows_per_gpu, S, A, seed=1000 + rank)
    replay = PackedReplay(shard, S, A, dev, rank=0, world=1, seed=rank)
    del shard
    _apply_tuning_env(E)

    def barrier():
        if dp:
            dist.barrier()
        torch.cuda.synchronize()

    # Set-up, not warm-up: ~50 ms of fp32-MFMA work on scratch tensors so that a short run (the driver times 20 steps
    # after 5 warm-up steps: 9 ms in all) does not measure the card's clock / power ramp from idle.  It touches no
    # agent state; the W warm-up updates and the K timed updates below are exactly as asked.  PORL_BENCH_SPINUP_MS=0
    # turns it off; the line states it as `setup_spinup_ms`.
    spin_ms = float(os.environ.get("PORL_BENCH_SPINUP_MS", "50"))

    def spinup():
        if spin_ms > 0:
            sa, sb = torch.randn(4096, 1024, device=dev), torch.randn(1024, 1024, device=dev)
            sc = torch.empty(4096, 1024, device=dev)
            t_spin = time.perf_counter()
            while (time.perf_counter() - t_spin) * 1e3 < spin_ms:
                for _ in range(20):
                    E.gemm_f32(0, sa, sb, 4096, 1024, 1024, 1024, 1024, sc, 1024)
                torch.cuda.synchronize()

    def make_agent(mode):
        args = SimpleNamespace(state_size=S, hidden_dim=H, n_hidden=L, layer_norm=False, action_size=A, max_batch=B)
        torch.manual_seed(0)                                       # identical replicas on every rank
        agent = POR(args, max_steps=1000, tau=0.9, alpha=10.0, device=dev)
        agent.async_losses = mode != "sync"                        # "sync": the reference's convention (floats back, one host sync per update)
        agent.pipeline = mode in ("pipelined", "reduce_scatter_pipelined_1comm", "reduce_scatter_pipelined_2comm")
        agent.grad_exchange = "all_reduce" if mode == "allreduce_1stream" else "reduce_scatter"
        agent.dp_policy_group = mode == "reduce_scatter_pipelined_2comm"
        return agent

    def timed_run(mode, steps, warmup, keep=False):
        """W warm-up updates, then exactly K timed updates bracketed by barrier + device synchronisation; MAX over ranks."""
        prio = os.environ.get("PORL_BENCH_MAIN_PRIORITY")            # A/B: the value phase's stream at another priority
        if prio is not None and not getattr(timed_run, "_in_prio", False):
            timed_run._in_prio = True
            try:
                with torch.cuda.stream(torch.cuda.Stream(device=dev, priority=int(prio))):
                    return timed_run(mode, steps, warmup, keep)
            finally:
                timed_run._in_prio = False
        agent = make_agent(mode)
        replay.draws = 0
        losses = torch.zeros(steps + warmup, 8, device=dev)       # device-side loss history, one row per update

        def one_step(i):
            # draw B distinct rows of the resident shard + gather + split (one kernel), then the update;
            # the three loss statistics of update i land in losses[i] without copies
            agent._engine.set_stats(losses[i])
            agent.update_from_replay(replay, B)

        # set-up spin-up HERE, after the agent has been built (allocation and initialisation leave the card idle for
        # ~0.1 s, long enough for it to fall back to its idle clocks): same-box comparison with scripts/bench_ramp.py,
        # which spins right before its warm-up updates — 2 965-3 079 updates/s for K = 20 against 2 777-2 852 with the
        # spin-up in front of the agent's construction (gpurun_out/r03/ramp)
        import gc
        gc.collect()                                               # (before the spin-up: a collection between warm-up and the
        gc.disable()                                               #  timed loop is 20 ms of idle card — 2 690 instead of 2 990)
        try:                                                       # no collector pause inside a 7 ms timed window
            spinup()
            for i in range(warmup):
                one_step(i)
            barrier()
            t0 = time.perf_counter()
            for i in range(steps):
                one_step(warmup + i)
            agent.flush()                                          # a deferred policy step belongs to the timed work
            barrier()
            elapsed = time.perf_counter() - t0
        finally:
            gc.enable()
        if dp:
            t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
            if agent.async_losses:
                # async mode keeps per-rank SHARES of the batch means in the history: one reduction after the timed
                # loop makes them the global-batch statistics (sum of shares; minimum of the per-rank minima)
                sums = losses[:, 0:2].contiguous()
                dist.all_reduce(sums, op=dist.ReduceOp.SUM)
                losses[:, 0:2] = sums
                mins = losses[:, 2].contiguous()
                dist.all_reduce(mins, op=dist.ReduceOp.MIN)
                losses[:, 2] = mins
        lh = losses[:, :3].cpu().numpy()
        if not np.isfinite(lh).all():
            raise SystemExit(f"non-finite loss in the benchmark run (mode {mode})")
        res = dict(mode=mode, elapsed=elapsed, steps_per_s=steps / elapsed, lh=lh, one_step=one_step, agent=agent)
        if not keep:
            res["agent"] = res["one_step"] = None
            del agent
        return res

    def line_for(res, steps, warmup):
        steps_per_s = res["steps_per_s"]
        # weak scaling: every rank pushes one batch-1024 through the update per step, so the whole-job
        # figure counts batch-1024 units of all ranks; one optimizer step consumes `world` of them
        # (its gradient is the mean over the world*1024 rows).  At N=1 the two numbers coincide.
        units_per_s = steps_per_s * world
        lh = res["lh"]
        mode = res["mode"]
        return {
            "metric": "gradient-steps/sec (POR update, batch=%d)" % B,
            "value": units_per_s, "unit": "gradient-steps/sec", "n_gpus": world, "steps": steps,
            "warmup": warmup, "ms_per_step": 1e3 * res["elapsed"] / steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"POR S={S} A={A} H={H} L={L} B={B}/GPU (global {B * world}), "
                                   f"{rows_per_gpu * world} -row replay ({rows_per_gpu}/GPU) resident in HBM, "
                                   "device sampler + gather + full update per step",
                       "parallelism": f"dp{world}", "global_batch": B * world},
            "value_counts": "batch-%d units of all ranks per second (= optimizer steps/s x n_gpus: weak scaling)" % B,
            "optimizer_steps_per_sec": steps_per_s,
            "samples_per_sec": steps_per_s * B * world,
            "algorithmic_tflops": steps_per_s * B * world * por_flops_per_sample() / 1e12,
            "final_losses": {"v_loss": float(lh[-1, 0]), "g_loss": float(lh[-1, 1]), "min_nll": float(lh[-1, 2])},
            "update_mode": ("async_losses + two-stream pipelining (opt-in extensions, INTEGRATION.md); the reference's "
                            "synchronous convention is secondary.por_sync_mode of a --full run") if mode == "pipelined" else mode,
            "setup_spinup_ms": spin_ms,
            "rccl_ranks": dist.get_world_size() if dp else 1,
            "backend": (dist.get_backend() if dp else "none"),
        }

    inject = os.environ.get("PORL_BENCH_INJECT", "")                # tests: "die:<mode>" / "hang:<mode>"
    # -----------------------------------------------------------------------------------------------------------------
    if dp:
        modes = [m for m in (os.environ.get("PORL_BENCH_MODES") or ",".join(DP_MODES)).split(",") if m]
        results = []
        for mode in modes:
            if inject == "die:" + mode and rank == world - 1:
                os._exit(17)
            if inject == "hang:" + mode and rank == world - 1:
                time.sleep(3600)
            res = timed_run(mode, a.steps, a.warmup)
            ln = line_for(res, a.steps, a.warmup)
            ln["dp"] = dict(mode=mode, grad_exchange="all_reduce" if mode == "allreduce_1stream" else "reduce_scatter",
                            pipelined="pipelined" in mode, policy_process_group=mode.endswith("2comm"),
                            forced_on_one_rank=bool(force_dp and world == 1))
            results.append(dict(mode=mode, ok=True, value=ln["value"], ms_per_step=ln["ms_per_step"], line=ln))
            barrier()                                              # every rank has finished the mode before it is reported
            if rank == 0:
                print("PORL_MODE " + json.dumps(results[-1]), flush=True)
            print("PORL_MODE_DONE " + mode, flush=True)
        best = max(results, key=lambda r: r["value"])
        out = dict(best["line"])
        out["dp"] = dict(out["dp"], modes=[{k: v for k, v in r.items() if k != "line"} for r in results], failed=[],
                         order="conservative first; `value` = the best mode that finished")
        barrier()
        if rank == 0:
            print("PORL_FINAL " + json.dumps(out), flush=True)
        # nothing collective after the result: a rank that fails from here on cannot take the line with it
        try:
            dist.destroy_process_group()
        except Exception:
            pass
        return

    # ---- N = 1 ------------------------------------------------------------------------------------------------------
    mode = "one_stream" if a.no_pipeline else "pipelined"
    res = timed_run(mode, a.steps, a.warmup, keep=True)
    out = line_for(res, a.steps, a.warmup)
    agent, one_step = res["agent"], res["one_step"]
    if a.dump_outputs:
        # before anything below updates the agent again: [v_loss, g_loss, min_nll] of the last timed update and the
        # networks it left (value twins, their target, goal policy)
        dump_outputs(a.dump_outputs, {"losses": res["lh"][-1], **agent.state_dict()})

    # From here on --full only: the headline needs none of it.
    # Not `value`: the same loop again for 1 000 updates, five times, median.  The first ~20 updates after a device sync
    # run ~4 % slower than the steady state (scripts/bench_ramp.py: 315 against 303 us each) and a K = 20 run also pays the
    # pipeline's fill and drain (~0.3 ms) once; a training job runs millions of updates, so the sustained rate is reported
    # beside the contract's K-step figure.
    if a.full and a.steps < 1000 and os.environ.get("PORL_BENCH_SUSTAINED", "1") != "0":
        n_s, rates = 1000, []
        for _ in range(5):
            barrier()
            ts = time.perf_counter()
            for i in range(n_s):
                one_step(a.warmup + i % a.steps)
            agent.flush()
            barrier()
            rates.append(n_s / (time.perf_counter() - ts))
        out["sustained_1000_updates_per_sec"] = float(np.median(rates))
        out["sustained_runs"] = [round(r, 1) for r in rates]

    if a.full and not a.no_roofline:
        out["roofline"] = por_roofline(E, agent, one_step, a, mode)
    del agent, one_step, res

    if a.full and not a.no_secondary and H == 1024 and B == 1024:
        sec = {}
        t_sec = time.perf_counter()

        def guarded(name, fn):
            if time.perf_counter() - t_sec > float(os.environ.get("PORL_BENCH_SECONDARY_BUDGET_S", "150")):
                sec[name] = {"skipped": "secondary time budget used up"}
                return
            try:
                sec[name] = fn()
            except Exception as e:                                  # a secondary figure must never take the headline with it
                sec[name] = {"error": f"{type(e).__name__}: {e}"[:300]}
            torch.cuda.synchronize()

        def por_variant(mode_, steps, warmup):
            r = timed_run(mode_, steps, warmup)
            return dict(value=r["steps_per_s"], ms_per_step=1e3 * r["elapsed"] / steps, steps=steps, warmup=warmup)

        # the reference's calling convention, unchanged por_train.py:79-82: floats come back, one host sync per update
        guarded("por_sync_mode", lambda: dict(por_variant("sync", max(a.steps, 100), a.warmup),
                                              note="async_losses=False: everything on one stream, losses returned as "
                                                   "Python floats every update (what an unmodified por_train.py loop gets)"))
        guarded("por_one_stream", lambda: dict(por_variant("one_stream", max(a.steps, 100), a.warmup),
                                               note="async_losses=True, no two-stream pipelining"))

        def h256():
            global H
            keep = H
            H = 256
            try:
                r = por_variant("pipelined", max(a.steps, 200), max(a.warmup, 20))
                r["workload"] = "POR S=60 H=256 (class default, value_functions.py:32) L=2 B=1024, pipelined"
                return r
            finally:
                H = keep
        guarded("por_h256_b1024", h256)
        guarded("cql_b4096", lambda: _brief(measure_cql(max(a.steps, 200), max(a.warmup, 20), with_cpu=False)))
        guarded("sorl_enc_fp32_360x256_b512", lambda: _brief(measure_sorl_enc(max(10, min(a.steps, 20)), 3, 512, 360, 256, "fp32", False)))
        guarded("sorl_enc_bf16_84x84_b512", lambda: _brief(measure_sorl_enc(max(a.steps, 50), 5, 512, 84, 84, "bf16", False)))
        guarded("sorl_enc_bf16_360x256_b512", lambda: _brief(measure_sorl_enc(max(10, min(a.steps, 20)), 3, 512, 360, 256, "bf16", False)))
        out["secondary"] = sec

    if a.full and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline()
        out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
    print(json.dumps(out), flush=True)


def _apply_tuning_env(E):
    """A/B switches of DESIGN.md §5 (none is set in a default run)."""
    if os.environ.get("PORL_IQL_FOLD") == "0":                 # slab combines as separate launches
        E.tune_set("iql_fold", 0)
    if os.environ.get("PORL_L0_KERNEL") == "0":                # input layers through the grouped GEMM
        E.tune_set("l0_kernel", 0)
    for i, v in enumerate(os.environ.get("PORL_TILE_MAP", "").split(",")):      # e.g. "0,1,2,3" = round-1 choice
        if v.strip():
            E.tune_set("tile_map%d" % i, int(v))
            E.tune_set("tile_map_short%d" % i, int(v))
    if os.environ.get("PORL_IQL_PAD"):                         # "value,policy[,min_blocks]" LDS pads of the pipelined update
        v = [int(x) for x in os.environ["PORL_IQL_PAD"].split(",")]
        E.tune_set("iql_pad_value", v[0]); E.tune_set("iql_pad_policy", v[1])
        if len(v) > 2:
            E.tune_set("iql_pad_min_blocks", v[2])
        if len(v) > 3:
            E.tune_set("iql_pad_min_k", v[3])
    if os.environ.get("PORL_GEMM_LDS_PAD"):                    # fewer co-resident GEMM blocks per CU (placement knob)
        E.tune_set("gemm_lds_pad", int(os.environ["PORL_GEMM_LDS_PAD"]))
    if os.environ.get("PORL_VBWD_TILE"):                       # tile of the value backward in pipelined mode
        E.tune_set("vbwd_tile_short", int(os.environ["PORL_VBWD_TILE"]))
    if os.environ.get("PORL_L0_TILE"):                         # tile of the K = 60 forward layers
        E.tune_set("l0_tile", int(os.environ["PORL_L0_TILE"]))
    for kv in os.environ.get("PORL_TUNE", "").split(","):      # generic: "key=value,key=value"
        if "=" in kv:
            k, v = kv.split("=")
            E.tune_set(k.strip(), int(v))


def por_roofline(E, agent, one_step, a, mode):
    """Second pass, instrumented: HIP events around every kernel launch on the launch stream.  The timed loop overlaps
    the policy phase with the next value phase on two streams; a kernel's roofline is quoted with the kernel ALONE on
    the chip, so this pass runs the same updates back to back on one stream."""
    agent.flush()
    agent.pipeline = False
    psteps = max(a.steps, 100)                 # enough launches for stable per-kernel averages whatever K is
    E.prof_enable(True)
    for i in range(psteps):
        one_step(a.warmup + i % a.steps)
    prof = E.prof_read()
    E.prof_enable(False)
    agent.pipeline = mode == "pipelined"
    # profile labels are "<launch of the step>:<kernel>".  The roofline is quoted for the DOMINANT LAUNCH of the
    # update (the labelled launch with the largest total time: the 4-net hidden-layer forward) — one kernel
    # instantiation can serve launches of very different shapes, which a per-instantiation average would mix
    gemms = [p for p in prof if p["launches"] and "gemm_f32_kernel" in p["name"]]
    if not gemms:
        return None
    dom = max(gemms, key=lambda p: p["total_ms"])
    name = dom["name"].split(":")[-1]
    avg_ms = dom["total_ms"] / dom["launches"]
    flops_per_launch = dom["flops"] / dom["launches"]
    ach = flops_per_launch / (avg_ms * 1e-3) / 1e12
    # HBM bytes per launch are NOT measured by this run: they come from the committed rocprofv3 --pmc passes
    # over this same command (separate passes, as the microarch guide prescribes); the source file is named
    traffic, traffic_src = None, None
    for fname in ("r03_hbm_traffic.json", "r02_hbm_traffic.json", "r01_hbm_traffic.json"):
        try:
            tj = json.load(open(os.path.join(REPO, "profiles", fname)))
            traffic = tj["kernels"][name]["hbm_bytes_per_launch"]
            traffic_src = "profiles/" + fname
            break
        except Exception:
            pass
    small = [p for p in prof if p["launches"] and p["flops"] / max(1, p["launches"]) < 2e9]
    roof = dict(bound="mfma", kernel=name, launch=dom["name"], achieved=ach, peak=PEAK_FP32_MFMA_TFLOPS, unit="TFLOP/s",
                frac=ach / PEAK_FP32_MFMA_TFLOPS, traffic=traffic, traffic_source=traffic_src,
                avg_launch_us=avg_ms * 1e3, launches=dom["launches"],
                flop_per_launch=flops_per_launch,
                launches_per_step=sum(p["launches"] for p in prof) / psteps,
                instrumented_pass="%d updates back to back on one stream (no overlap), HIP events around "
                                  "every launch (~2.5 us of event overhead inside each figure)" % psteps,
                step_sum_us=round(sum(1e3 * p["total_ms"] / psteps for p in prof if p["launches"]), 2),
                small_launches_us=round(sum(1e3 * p["total_ms"] / psteps for p in small), 2),
                # every launch of one update, HIP-event timed on the launch stream (instrumented pass)
                step_launches_us={p["name"]: round(1e3 * p["total_ms"] / psteps, 2) for p in prof if p["launches"]})
    # SURVEY.md §8(d) asks for both fractions: the HBM-bound launch of the update is the value group's
    # Adam + Polyak sweep (36 B per parameter + the folded slab combines, algorithmic bytes from the launch site)
    sweeps = [p for p in prof if p["launches"] and "adam_ema_kernel" in p["name"] and p["bytes"] > 0]
    if sweeps:
        sw = max(sweeps, key=lambda p: p["bytes"])
        sw_ms = sw["total_ms"] / sw["launches"]
        gbs = sw["bytes"] / sw["launches"] / (sw_ms * 1e-3) / 1e9
        roof["hbm_bound_launch"] = dict(bound="hbm", launch=sw["name"], achieved=gbs, peak=PEAK_HBM_GBS, unit="GB/s",
                                        frac=gbs / PEAK_HBM_GBS, avg_launch_us=sw_ms * 1e3,
                                        bytes_per_launch=sw["bytes"] / sw["launches"])
    return roof


if __name__ == "__main__":
    main()
