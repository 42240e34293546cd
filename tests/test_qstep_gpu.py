"""The Q-network learn step, per row and per gradient element, against the fp64 oracle of tests/helpers/qstep_cases.py, on
every kernel form: the three one-launch kernels of csrc/qnet_fused.hpp (`fused16` = qnet_fused2_kernel<16>, the default;
`fused2` = qnet_fused2_kernel<32>; `fused1` = qnet_fused_kernel) and the multi-launch path of csrc/qnet_api.inc with
cql_loss_kernel (`general`).  One learn_indexed per case on a minibatch of decided rows (no row is left out), then:
td_abs, stats[0..2] and every gradient tensor against step64 at  max(2e-6, 2 x the fp32 control's error on the same case)
(errors as qstep_cases.errors defines them); the bootstrap action in the tie case and in the all-zero mask row; the Adam
fold against adam64 on the engine's own gradient buffer; the zero padding of the parameter images; params_tgt untouched.

The bars are not tuned against the kernels.  Largest observed error / bar per form (MI355X), over the 177 cases; every
bar that decided was the 2e-6 floor:
    fused16  0.27  (row1-a5-double_dqn, output-layer bias gradient: 5.3e-7)
    fused2   0.30  (odd-a2-dqn, output-layer bias gradient: 6.0e-7)
    fused1   0.30  (bit-identical to fused2)
    general  0.31  (maxk-a5-cql, first-layer weight gradient: 6.2e-7)
(`maxk` leaves no room for a second weight image in LDS: its three one-launch forms all run qnet_fused_kernel.)

Hand mutations of csrc/qnet_fused.hpp these tests were tried against: `wgt` dropped from the j == act term of
qf_loss_rows8 (fails every shape; of the older tests only the PER golden); `>=` in the amax loops (fails the tie case; the
older tests pass); the plain maximum instead of the masked pick in qf_loss_row_regs<6> (fails odd at A = 17 and 24; the
older tests pass); the reduce loop's second trip started at slab j + 56 (fails fused16-blocks; the older tests see it at
B = 4096); dead rows of the loop branch left unzeroed in the action columns (fails every shape).  Not zeroing dq[A..ldq)
of a live row in the loop branch changes no result: those columns only ever meet the zero rows of the weight image's
padding, which the padding check here keeps at zero — the store guards against non-finite leftovers in LDS only.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from helpers import qstep_cases as Q
from porl_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLOOR, CONTROL_FACTOR = 2e-6, 2.0
SENTINEL = -7.25
PAD = 64
# tuning keys a form sets before its engines are built (an existing engine keeps its selection); defaults are all 1
FORMS = {"fused16": {}, "fused2": {"qnet_rows16": 0}, "fused1": {"qnet_two_groups": 0}, "general": {"qnet_fused": 0}}
TUNE_DEFAULTS = {"qnet_rows16": 1, "qnet_two_groups": 1, "qnet_fused": 1}


@contextlib.contextmanager
def _form(form):
    from porl_amd import engine as E
    try:
        for k, v in FORMS[form].items():
            E.tune_set(k, v)
        yield
    finally:
        for k, v in TUNE_DEFAULTS.items():
            E.tune_set(k, v)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(inputs, fp64 step, fp32 control's errors) of a case: computed once, shared by every form, never modified."""
    d = Q.make(Q.BY_NAME[name])
    r64 = Q.step64(d)
    return d, r64, Q.errors(r64, Q.step32(d))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _engine(case):
    from porl_amd.train.cql_trainer import QnetEngine
    return QnetEngine(case["S"], case["A"], case["hidden"], max(case["B"], 64), DEV)


def _write_state(eng, d):
    """Parameters and moments through the tensor views: the images' padding is never written from here."""
    for flat, src in ((eng.params, d["online"]), (eng.params_tgt, d["target"]), (eng.adam_m, d["adam_m"]), (eng.adam_v, d["adam_v"])):
        for view, arr in zip(eng.views(flat), src):
            view.copy_(_dev(arr))


def _arena(*arrays):
    """The arrays side by side in one buffer, PAD sentinel floats before, between and after them -> (buffer, views)."""
    n = PAD + sum(a.size + PAD for a in arrays)
    host = np.full(n, SENTINEL, dtype=np.float32)
    spans, o = [], PAD
    for a in arrays:
        host[o:o + a.size] = np.asarray(a, dtype=np.float32).ravel()
        spans.append((o, a.size))
        o += a.size + PAD
    buf = _dev(host)
    return buf, host, [buf[o:o + n_] for o, n_ in spans]


def _variant(d, td_abs=None):
    """(QnetVariant or None, read-only argument arena and its host image)."""
    v = Q.variant(d["case"])
    buf, host, (is_w, w_u, mask) = _arena(d["is_w"], np.array([d["w_uniform"]], dtype=np.float32), d["mask"])
    if not (v["double_dqn"] or v["is_w"] or v["w_uniform"] or v["mask"] or v["td_off"] or td_abs is not None):
        return None, buf, host                                     # plain CQL / DQN: porl_qnet_learn_indexed
    var = N.QnetVariant(int(v["double_dqn"]), N.ptr(is_w) if v["is_w"] else None, N.ptr(w_u) if v["w_uniform"] else None,
                        N.ptr(td_abs) if td_abs is not None else None, N.ptr(mask) if v["mask"] else None, int(v["td_off"]))
    return var, buf, host


def _run(eng, d, with_td_abs):
    """One learn step of the case on `eng` -> everything the step wrote, on the host."""
    case, v = d["case"], Q.variant(d["case"])
    B = case["B"]
    _write_state(eng, d)
    before = {k: getattr(eng, k).clone() for k in ("params", "params_tgt", "adam_m", "adam_v")}
    replay = [_dev(d[k]) for k in ("states", "actions", "rewards", "next_states", "dones")]
    td_buf = torch.full((B + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    td = td_buf[PAD:PAD + B] if with_td_abs else None
    var, arena, arena_host = _variant(d, td)
    hp = eng.hyper(Q.GAMMA, v["alpha"], 1.0 / B, Q.STEP, Q.LR, Q.BETAS, Q.EPS)
    eng.learn_indexed(hp, *replay, _dev(d["idx"]), variant=var)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(arena.cpu().numpy(), arena_host, err_msg="the step wrote to its read-only arguments")
    td_host = td_buf.cpu().numpy()
    assert (td_host[:PAD] == SENTINEL).all() and (td_host[PAD + B:] == SENTINEL).all(), "td_abs written outside [0, B)"
    if not with_td_abs:
        assert (td_host == SENTINEL).all()
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in ("params", "params_tgt", "adam_m", "adam_v", "grads")}
    out["stats"] = eng.stats[:3].cpu().numpy().copy()
    out["td_abs"] = td_host[PAD:PAD + B].copy()
    out["before"] = {k: x.cpu().numpy() for k, x in before.items()}
    return out


def _tensors(eng, flat):
    """The tensors of a flat host image, in tensor_table order."""
    out = []
    for off, shape, ld in eng.tensor_table():
        out.append(flat[off:off + shape[0]].copy() if len(shape) == 1
                   else flat[off:off + shape[0] * ld].reshape(shape[0], ld)[:, :shape[1]].copy())
    return out


def _cover(eng):
    cover = np.zeros(eng.n_params, dtype=bool)
    for off, shape, ld in eng.tensor_table():
        if len(shape) == 1:
            cover[off:off + shape[0]] = True
        else:
            cover[off:off + shape[0] * ld].reshape(shape[0], ld)[:, :shape[1]] = True
    return cover


def _check_step(eng, d, r64, control, out, with_td_abs):
    """-> [(quantity, error, bar)] of one case; raises on everything that is exact."""
    case, v = d["case"], Q.variant(d["case"])
    B = case["B"]
    assert np.isfinite(out["grads"]).all() and np.isfinite(out["stats"]).all()
    got = dict(td_abs=out["td_abs"] if with_td_abs else r64["td_abs"], stats=out["stats"], grads=_tensors(eng, out["grads"]))
    err = Q.errors(r64, got)
    bar = lambda c: max(FLOOR, CONTROL_FACTOR * c)
    rows = [("stats", err["stats"], bar(control["stats"]))]
    if with_td_abs:
        rows.append(("td_abs", err["td_abs"], bar(control["td_abs"])))
    rows += [(f"grad[{i}]", e, bar(c)) for i, (e, c) in enumerate(zip(err["grads"], control["grads"]))]
    # the bootstrap action, read off td_abs
    if with_td_abs and case["tie"]:
        live = d["tie_rows"] & (d["dones"][d["idx"]] == 0)
        first, second = (Q.td_abs_for_action(d, r64, j) for j in Q.TIE_PAIR)
        assert live.sum() >= 3
        assert (np.abs(out["td_abs"] - first)[live] < np.abs(out["td_abs"] - second)[live]).all(), "tie: not the first maximum"
    if with_td_abs and v["mask"] and B >= 3:
        zero = Q.td_abs_for_action(d, r64, 0)
        plain = Q.td_abs_for_action(d, r64, int(r64["q_target_next"][1].argmax()))
        assert abs(out["td_abs"][1] - zero[1]) < abs(out["td_abs"][1] - plain[1]), "all-zero mask row: not action 0"
        assert abs(out["td_abs"][1] - zero[1]) <= bar(control["td_abs"]) * max(1.0, float(r64["td_abs"].max()))
    # Adam: the fold of the engine's OWN gradient buffer into parameters and moments
    b = out["before"]
    p, m, vv = Q.adam64(b["params"], out["grads"], b["adam_m"], b["adam_v"])
    np.testing.assert_allclose(out["params"], p, atol=1e-7, rtol=1e-6, err_msg="params after Adam")
    np.testing.assert_allclose(out["adam_m"], m, atol=1e-9, rtol=1e-5, err_msg="adam_m")
    np.testing.assert_allclose(out["adam_v"], vv, atol=1e-12, rtol=1e-5, err_msg="adam_v")
    # padding of the images stays exactly zero; the target network is not touched
    pad = ~_cover(eng)
    for k in ("params", "grads", "adam_m", "adam_v"):
        assert not out[k][pad].any(), f"{k}: non-zero padding"
    assert out["params_tgt"].tobytes() == b["params_tgt"].tobytes()
    return rows


@pytest.mark.parametrize("shape", list(Q.SHAPES))
@pytest.mark.parametrize("form", list(FORMS))
def test_step_matches_fp64_oracle(form, shape):
    cases = [c for c in Q.CASES if c["shape"] == shape]
    assert cases
    worst, failed = (0.0, None), []
    with _form(form):
        engines = {}
        for case in cases:
            d, r64, control = _ref(case["name"])
            # one engine per output width, reused by its variants: the padding has to stay zero across their steps too
            eng = engines.get(case["A"])
            if eng is None:
                eng = engines[case["A"]] = _engine(case)
            assert eng.fused == (form != "general"), case["name"]
            with_td = Q.variant(case)["td_abs"]
            try:
                rows = _check_step(eng, d, r64, control, _run(eng, d, with_td), with_td)
            except AssertionError as e:
                failed.append(f"{case['name']}: {str(e).strip().splitlines()[0] if str(e).strip() else 'assert'}")
                continue
            for what, e, bar in rows:
                if e / bar > worst[0]:
                    worst = (e / bar, f"{case['name']} {what} err {e:.3g} bar {bar:.3g}")
                if not e <= bar:
                    failed.append(f"{case['name']} {what}: error {e:.3g} > bar {bar:.3g}")
    print(f"\n[qstep] {form} {shape}: {len(cases)} cases, worst error/bar {worst[0]:.3f} ({worst[1]})")
    assert not failed, f"{len(failed)} failures:\n" + "\n".join(failed[:40])


@pytest.mark.parametrize("var", ["double_dqn", "bcq_mask"])
def test_more_than_128_outputs_take_the_multi_launch_path(var):
    """The output-width contract of include/porl_hip.h: 128 outputs are the one-launch kernels' last width (the grid above
    runs it), 129 go to the multi-launch path by themselves and are held to the same oracle there."""
    d128 = Q.BY_NAME[f"odd-a128-{var}"]
    assert _engine(d128).fused
    d = Q.make(Q.case("odd", 129, var))
    r64 = Q.step64(d)
    eng = _engine(d["case"])
    assert not eng.fused and not eng.can_sample
    for what, e, bar in _check_step(eng, d, r64, Q.errors(r64, Q.step32(d)), _run(eng, d, True), True):
        assert e <= bar, (what, e, bar)


@pytest.mark.parametrize("name", ["odd-a5-cql", "odd-a33-dqn", "odd-a5-both_weights", "odd-a33-both_weights"])
@pytest.mark.parametrize("form", list(FORMS))
def test_td_abs_is_optional_and_written_nowhere_else(form, name):
    """Variants that do not ask for td_abs: without the pointer nothing is written (sentinels around every argument); with it
    the same step leaves the same bits everywhere else and |TD| per row against the oracle."""
    d, r64, control = _ref(name)
    with _form(form):
        a, b = _engine(d["case"]), _engine(d["case"])
        without, with_ = _run(a, d, False), _run(b, d, True)
        rows = _check_step(b, d, r64, control, with_, True)
    for k in ("params", "adam_m", "adam_v", "grads", "stats"):
        assert without[k].tobytes() == with_[k].tobytes(), k
    for what, e, bar in rows:
        assert e <= bar, (what, e, bar)


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("var", ["cql", "per"])
def test_in_kernel_sampler_on_ragged_batches(var, B):
    """learn_sampled (with and without a variant) on a batch that does not fill its last block: bit-equal to learn_indexed on the
    rows engine.sample_indices gives; is_w and td_abs are indexed by minibatch position."""
    from porl_amd import engine as E
    d, _, _ = _ref(f"{'row1' if B == 1 else 'odd'}-a5-{var}")
    case, v = d["case"], Q.variant(d["case"])
    assert case["B"] == B
    seed, draw, n_rows = 11, 2, d["n_rows"]
    replay = [_dev(d[k]) for k in ("states", "actions", "rewards", "next_states", "dones")]
    out = []
    for sampled in (True, False):
        eng = _engine(case)
        assert eng.fused and eng.can_sample
        _write_state(eng, d)
        td = torch.full((B + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
        var_, arena, arena_host = _variant(d, td if v["td_abs"] else None)
        hp = eng.hyper(Q.GAMMA, v["alpha"], 1.0 / B, Q.STEP, Q.LR, Q.BETAS, Q.EPS)
        if not sampled:
            idx = E.sample_indices(n_rows, B, seed, draw, device=DEV)
            assert len(set(idx.tolist())) == B and 0 <= int(idx.min()) and int(idx.max()) < n_rows
            eng.learn_indexed(hp, *replay, idx, variant=var_)
        else:
            eng.learn_sampled(hp, *replay, n_rows, B, seed, draw, variant=var_)
        torch.cuda.synchronize()
        assert (td[B:] == SENTINEL).all()
        assert bool((td[:B] != SENTINEL).all()) == v["td_abs"]
        out.append([x.clone() for x in (eng.params, eng.adam_m, eng.adam_v, eng.grads, eng.stats[:3], td)])
    for x, y, what in zip(out[0], out[1], ("params", "adam_m", "adam_v", "grads", "stats", "td_abs")):
        assert torch.equal(x, y), what
    assert float(out[0][3].abs().max()) > 0
