"""Writes tests/golden/iql_launches.json: which labelled launches every IQL-engine entry point issues, per case.

    python tests/helpers/gen_iql_launches.py

Needs a GPU and the built library.  Run at the commit whose host code is the yardstick (the fixture was recorded before
the engine moved to csrc/iql_api.inc); tests/test_iql_launches_gpu.py replays every case on the current build and
compares exactly, tests/test_iql_launches.py (no GPU) checks that the fixture names the cases listed here.

A case is a network shape, a call pattern and kernel-selection keys.  Its record is the ordered list of entry-point
calls, each with the profile labels (g_phase prefix included) that porl_prof_read reports for that call and how often
each was launched.  porl_prof_read keeps one row per label, so inside one call the order is that of the phase prefixes
(V2. < V3. < ...), which is why the labels of a call are stored sorted; the order of the calls is the pattern's.
Launches without a profile label (pack_kernel, the LayerNorm kernels, value_loss_kernel, the finish kernels) do not
appear.  Host decisions depend on shapes, modes and tuning keys only, never on the numbers in the buffers.
"""
import json
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(os.path.dirname(HERE), "golden", "iql_launches.json")

# weight_mode 1 regresses the action (D = act_dim), 0 the next state (D = S)
SHAPES = {
    "s11": dict(S=11, D=3, H=64, L=1, B=8, ln=0, wm=1),       # one hidden layer: layer 0 is also the last
    "s17": dict(S=17, D=3, H=256, L=2, B=256, ln=0, wm=1),    # several blocks per launch, split-K below the chip's width
    "ln": dict(S=17, D=3, H=132, L=3, B=33, ln=1, wm=1),      # LayerNorm twins, odd batch, three layers (both ping-pong halves)
    "s12": dict(S=12, D=3, H=64, L=2, B=40, ln=0, wm=1),      # S % 4 == 0 and S <= 64: layer 0 on l0_fwd_kernel
    "s70": dict(S=70, D=70, H=128, L=2, B=64, ln=0, wm=0),    # S > 64: no l0 kernel, no skinny dW0; D > 64: GEMM output layer
}
TWO_SLOTS, FOLD_COMBINE, SHORT_BLOCKS = 1, 2, 4


def _hp(eng, B, u):
    return eng.hyper(inv_batch=1.0 / B, value_step=u, policy_step=u)


def _load(eng, d):
    return [("load_batch", lambda: eng.load_batch(d.obs, d.next, d.rew, d.term, d.target))]


def _value(eng, d, u):
    hp = _hp(eng, d.B, u)
    return [("value_backward", lambda: eng.value_backward(hp)), ("value_apply", lambda: eng.value_apply(hp))]


def _policy(eng, d, u, forward=True):
    hp = _hp(eng, d.B, u)
    return ([("policy_forward", lambda: eng.policy_forward(hp))] if forward else []) + \
        [("policy_backward", lambda: eng.policy_backward(hp)), ("policy_apply", lambda: eng.policy_apply(hp))]


def p_phases(eng, d, u):
    return _load(eng, d) + _value(eng, d, u) + _policy(eng, d, u)


def p_phases_joint_backward(eng, d, u):
    """policy_backward without policy_forward: the forward half runs inside it."""
    return _load(eng, d) + _value(eng, d, u) + _policy(eng, d, u, forward=False)


def p_step(eng, d, u):
    hp = _hp(eng, d.B, u)
    return _load(eng, d) + [("step", lambda: eng.step(hp))]


def p_prefetch_phases(eng, d, u):
    return _load(eng, d) + _value(eng, d, u) + [("policy_prefetch", eng.policy_prefetch)] + _policy(eng, d, u)


def p_prefetch_backward(eng, d, u):
    return _load(eng, d) + _value(eng, d, u) + [("policy_prefetch", eng.policy_prefetch)] + _policy(eng, d, u, forward=False)


def p_prefetch_step(eng, d, u):
    hp = _hp(eng, d.B, u)
    return _load(eng, d) + [("policy_prefetch", eng.policy_prefetch), ("step", lambda: eng.step(hp))]


def p_policy_only(eng, d, u):
    hp = _hp(eng, d.B, u)
    return _load(eng, d) + [("policy_only_step", lambda: eng.policy_only(hp))]


def p_prefetch_policy_only(eng, d, u):
    hp = _hp(eng, d.B, u)
    return _load(eng, d) + [("policy_prefetch", eng.policy_prefetch), ("policy_only_step", lambda: eng.policy_only(hp))]


def p_policy_only_split(eng, d, u):
    hp = _hp(eng, d.B, u)
    return _load(eng, d) + [("policy_only_forward", lambda: eng.policy_only_forward(hp))] + _policy(eng, d, u, forward=False)


def p_pipelined(eng, d, u):
    """What agent/_iql.py passes in its default ordering mode: no slot wait, the forward-half wait from update 2 on."""
    hp = _hp(eng, d.B, u)

    def call():
        eng.update_pipelined(hp, d.replay, d.B, u, 0, u - 1, False)
        d.replay.draws += 1
    return [("update_pipelined", call)]


def p_load_no_target(eng, d, u):
    return [("load_batch", lambda: eng.load_batch(d.obs, d.next, d.rew, d.term, None))] + _value(eng, d, u)


def p_load_sampled(eng, d, u):
    hp = _hp(eng, d.B, u)
    return [("load_batch_sampled", lambda: eng.load_batch_sampled(d.rows, d.B, 1234, u, d.A, d.wm == 1)),
            ("step", lambda: eng.step(hp))]


def p_load_indexed(eng, d, u):
    hp = _hp(eng, d.B, u)
    return [("load_batch_indexed", lambda: eng.load_batch_indexed(d.rows, d.idx, d.S, d.A, d.wm == 1)),
            ("step", lambda: eng.step(hp))]


def p_load_indexed_features(eng, d, u):
    hp = _hp(eng, d.B, u)
    return [("load_batch_indexed", lambda: eng.load_batch_indexed(d.rows5, d.idx, 5, d.A, True, d.obs, d.next)),
            ("step", lambda: eng.step(hp))]


def p_forwards(eng, d, u):
    """B <= 8 takes the small-batch kernels, more the batched path (test_forward_gpu.py pins their arithmetic)."""
    out = []
    for n in sorted({min(8, d.B), max(9, d.B)}):
        x = d.wide[:n]
        out += [(f"forward_value[{n}]", lambda x=x: eng.forward_value(x)),
                (f"forward_value_target[{n}]", lambda x=x: eng.forward_value(x, target=True)),
                (f"forward_policy[{n}]", lambda x=x: eng.forward_policy(x))]
    return out


PATTERNS = {f.__name__[2:]: f for f in (
    p_phases, p_phases_joint_backward, p_step, p_prefetch_phases, p_prefetch_backward, p_prefetch_step, p_policy_only,
    p_prefetch_policy_only, p_policy_only_split, p_pipelined, p_load_no_target, p_load_sampled, p_load_indexed,
    p_load_indexed_features, p_forwards)}


def _case(shape, pattern, covers, mode=0, tune=(), tag=""):
    name = f"{shape}-{pattern}" + (f"-{tag}" if tag else "")
    return SimpleNamespace(name=name, shape=shape, pattern=pattern, mode=mode, tune=tuple(tune), covers=covers)


PIPE = TWO_SLOTS | FOLD_COMBINE | SHORT_BLOCKS
# `covers`: the shared host step (csrc/iql_api.inc) and the branch of it that the case is there for
CASES = [
    _case("s11", "phases", "twin / policy FwdNet with layer 0 == last layer (no stored output, head in the epilogue); skinny dW0 of 2 + 1 nets; out_bwd_kernel"),
    _case("s17", "phases", "S % 4 != 0: layer 0 through the grouped GEMM; masked per-layer backward group; combine launches of their own"),
    _case("ln", "phases", "LayerNorm twins: value_loss_kernel path, unmasked backward group, per-layer combines, grouped split-K dW0"),
    _case("s70", "phases", "S > 64: layer 0 through the grouped GEMM, dW0 split-K slabs (value twins and policy); D > 64: mean and output layer on the GEMM, slab_b"),
    _case("s12", "phases", "l0_fwd_kernel for the 4 value nets and for 2 twins + policy"),
    _case("s12", "prefetch_phases", "l0_fwd_kernel for the policy net alone and for the 2 twins"),
    _case("s12", "policy_only", "l0_fwd_kernel: 5 nets of the policy-only forward"),
    _case("s12", "pipelined", "l0_fwd_kernel inside the pipelined update", mode=PIPE),
    _case("s12", "phases", "l0_kernel off on a shape that would take it", tune=[("l0_kernel", 0)], tag="nol0"),
    _case("s12", "forwards", "l0_fwd_kernel for 2 twins / the policy net in the batched forwards"),
    _case("s11", "phases_joint_backward", "policy_backward running the joint forward half itself"),
    _case("s70", "phases_joint_backward", "the same with the GEMM mean"),
    _case("s11", "step", "value_adam / policy_adam with the combines folded"),
    _case("s17", "step", "the same, several layers"),
    _case("ln", "step", "LayerNorm: only the last combine is deferred"),
    _case("s70", "step", "split-K slabs folded into Adam"),
    _case("s17", "step", "iql_fold off: combines as launches, Adam without jobs", tune=[("iql_fold", 0)], tag="nofold"),
    _case("ln", "step", "the same with LayerNorm", tune=[("iql_fold", 0)], tag="nofold"),
    _case("s17", "prefetch_phases", "policy_fwd_net from the prefetch; joint forward with 2 nets and no mean launch"),
    _case("s70", "prefetch_phases", "the same on the GEMM layer 0 / GEMM mean (pol_nslab carried over)"),
    _case("s11", "prefetch_backward", "prefetch, then policy_backward doing both halves"),
    _case("ln", "prefetch_backward", "the same with LayerNorm twins"),
    _case("s17", "prefetch_step", "prefetch consumed by the one-call step"),
    _case("s11", "policy_only", "policy-only forward, 5 nets per layer, L = 1; O9 Adam"),
    _case("s17", "policy_only", "policy-only forward: 5 nets exceed the l0 kernel"),
    _case("ln", "policy_only", "policy-only forward with LayerNorm twins"),
    _case("s70", "policy_only", "policy-only with weight_mode 0 and the GEMM output layer"),
    _case("s17", "prefetch_policy_only", "policy-only forward with the policy net left out (4 nets)"),
    _case("s17", "policy_only_split", "policy_only_forward, then the ordinary gradient half and apply"),
    _case("ln", "policy_only_split", "the same with LayerNorm twins"),
    _case("s17", "phases", "FOLD_COMBINE: combines pending from *_backward to *_apply", mode=FOLD_COMBINE, tag="foldcombine"),
    _case("ln", "phases", "FOLD_COMBINE with LayerNorm", mode=FOLD_COMBINE, tag="foldcombine"),
    _case("s70", "phases", "FOLD_COMBINE with split-K slabs", mode=FOLD_COMBINE, tag="foldcombine"),
    _case("s17", "phases", "SHORT_BLOCKS: short tile map, LDS pad, skinny by width", mode=SHORT_BLOCKS, tag="short"),
    _case("s70", "phases", "SHORT_BLOCKS on the GEMM-only shape", mode=SHORT_BLOCKS, tag="short"),
    _case("s17", "phases", "SHORT_BLOCKS with skinny_pipelined 0 and a tile for the value backward", mode=SHORT_BLOCKS,
          tune=[("skinny_pipelined", 0), ("vbwd_tile_short", 3)], tag="short_noskinny"),
    _case("s11", "phases", "skinny off: grouped dW0 (split-K or not), GEMM mean, GEMM output layer at D <= 64", tune=[("skinny", 0)], tag="noskinny"),
    _case("s17", "phases", "the same at B = 256", tune=[("skinny", 0)], tag="noskinny"),
    _case("ln", "phases", "the same with LayerNorm twins", tune=[("skinny", 0)], tag="noskinny"),
    _case("s17", "policy_only", "policy-only with skinny off", tune=[("skinny", 0)], tag="noskinny"),
    _case("s17", "step", "skinny off, slabs folded into Adam", tune=[("skinny", 0)], tag="noskinny"),
    _case("s17", "phases", "l0_kernel off: layer 0 through the grouped GEMM", tune=[("l0_kernel", 0)], tag="nol0"),
    _case("ln", "phases", "l0_kernel off with LayerNorm", tune=[("l0_kernel", 0)], tag="nol0"),
    _case("s17", "policy_only", "l0_kernel off, policy-only", tune=[("l0_kernel", 0), ("l0_tile", 1)], tag="nol0_tile"),
    _case("s11", "pipelined", "one-call pipelined update, two in a row", mode=PIPE),
    _case("s17", "pipelined", "the same at B = 256", mode=PIPE),
    _case("ln", "pipelined", "the same with LayerNorm", mode=PIPE),
    _case("s70", "pipelined", "the same with weight_mode 0", mode=PIPE),
    _case("s17", "load_no_target", "load_batch without a policy target; value phase only"),
    _case("s17", "load_sampled", "porl_iql_load_batch_sampled, target = action"),
    _case("s70", "load_sampled", "porl_iql_load_batch_sampled, target = next state"),
    _case("s17", "load_indexed", "porl_iql_load_batch_indexed from raw rows"),
    _case("s70", "load_indexed", "the same, target = next state"),
    _case("s17", "load_indexed_features", "porl_iql_load_batch_indexed with feature matrices"),
    _case("s17", "load_sampled", "TWO_SLOTS: every load moves to the next slot", mode=TWO_SLOTS, tag="twoslots"),
    _case("s11", "forwards", "forward_value / forward_policy, small and batched"),
    _case("s17", "forwards", "the same at B = 256"),
    _case("ln", "forwards", "the same with LayerNorm (no small path for the twins)"),
    _case("s70", "forwards", "the same on GEMM layer 0 and GEMM mean"),
]
UPDATES = 2          # consecutive updates per case (the slot rotation and the pipelined waits differ between them)


def make_engine(case, device="cuda", seed=0):
    """A bound engine with seeded parameters, zeroed state and workspace, and the case's mode and tuning keys."""
    import torch
    from porl_amd.engine import IqlEngine
    s = SHAPES[case.shape]
    eng = IqlEngine(s["S"], s["D"], s["H"], s["L"], bool(s["ln"]), False, s["wm"], max_batch=max(9, s["B"]), device=device)
    g = torch.Generator().manual_seed(seed)
    for flat in (eng.params_vf, eng.params_tgt, eng.params_pol):
        flat.copy_(torch.randn(flat.numel(), generator=g) * 0.1)
    eng._ensure_bound()
    eng.workspace.zero_()
    eng.set_mode(case.mode)
    for k, v in case.tune:
        eng.tune_set(k, v)
    return eng


def make_data(case, device="cuda", seed=1):
    import torch
    s = SHAPES[case.shape]
    S, D, B = s["S"], s["D"], s["B"]
    A = D if s["wm"] == 1 else 2
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g).to(device)
    n_rows = 4 * B + 3
    d = SimpleNamespace(B=B, S=S, A=A, wm=s["wm"], obs=r(B, S), next=r(B, S), rew=r(B), term=(r(B) > 1).float(), target=r(B, D),
                        rows=r(n_rows, 2 * S + 2 + A + 1), rows5=r(n_rows, 2 * 5 + 2 + A), wide=r(max(9, B), S),
                        idx=torch.randperm(n_rows, generator=g)[:B].to(device))
    d.replay = SimpleNamespace(rows=d.rows, act_dim=A, seed=99, draws=0)
    return d


def run_case(case, observe, updates=UPDATES):
    """Runs the case's pattern `updates` times on a fresh engine; observe(eng, label, call) makes each entry-point call."""
    eng, d = make_engine(case), make_data(case)
    if case.pattern == "pipelined":
        eng.signals()
    for u in range(1, updates + 1):
        for label, call in PATTERNS[case.pattern](eng, d, u):
            observe(eng, f"{u}.{label}", call)
    import torch
    eng.join()
    torch.cuda.synchronize()


def record(case):
    """[[call, [[label, launches], ...]], ...] of one case."""
    from porl_amd import engine as E
    out = []

    def observe(eng, label, call):
        E.prof_enable(True)
        try:
            call()
            prof = E.prof_read(512)
        finally:
            E.prof_enable(False)
        out.append([label, sorted([p["name"], p["launches"]] for p in prof if p["launches"])])
    run_case(case, observe)
    return out


if __name__ == "__main__":
    golden = {}
    for c in CASES:
        golden[c.name] = record(c)
        print(c.name, sum(n for _, labels in golden[c.name] for _, n in labels), "labelled launches", flush=True)
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in golden.items()) + "\n}\n")
    print(f"{len(golden)} cases -> {OUT}")
