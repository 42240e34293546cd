"""The IQN engine (csrc/iqn_api.inc, the second half of csrc/iqn.hpp) against the fp64 oracle over the grid of
tests/helpers/iqn_cases.py, driven through porl_amd.engine.IqnEngine on flat buffers the test owns: parameters, target
parameters, Adam moments, the Adam step number and the fractions are all the case's.

Learn: the workspace is filled with NaN, then ONE eng.learn on a minibatch of decided samples (none is left out), then
    stats[0:3] (loss, total norm, clip coefficient) as relative errors against step64,
    each of the ten gradient tensors per element against step64's clipped gradient, over that tensor's largest fp64 entry,
each at  max(2e-6, 2 x the fp32 control's error for that quantity and case)  (2e-6: tests/test_qstep_gpu.py's allowance
for another summation order at equal precision); nothing is masked and no norm stands in for the per-element check.
Then, exactly or at fp32 rounding: the Adam launch against adam64 on the gradient read back from the device (so nothing
is amplified by 1 / (|g| + eps) and no entry is excused); the padding between the tensors of grads, params, adam_m and
adam_v exactly zero (the clip's sum of squares runs over the whole flat buffer); every gradient element overwritten;
params_tgt and the step's inputs bit-unchanged.  The same cases through IQNTrainer.learn_on (the autograd path) on `one`,
`ragged` and `tiles` meet the same bars, so that path sees H % 4 != 0 too.
Act: every state of every case, inline and as a device row, answers with the oracle's action; no state is skipped.

The bars are not tuned against the kernels.  Largest measured error / bar per quantity (MI355X, the 26 learn cases; the
bar is the 2e-6 floor unless a value follows), engine | autograd path:
    loss                        0.50 (wide, clipped: 1.7e-6 of 3.3e-6)   | 0.14
    total norm                  0.43 (wide: 1.0e-6 of 2.4e-6)            | 0.12
    clip coefficient            0.30 (fractions, clipped)                | 0.13
    feature_net.0.weight        0.63 (ragged A = 33: 1.8e-6 of 2.8e-6)   | 0.51
    feature_net.0.bias          0.56 (ragged A = 33: 2.1e-6 of 3.8e-6)   | 0.40
    feature_net.2.weight        0.57 (tiles)                             | 0.57
    feature_net.2.bias          0.51 (wide: 8.0e-6 of 1.6e-5)            | 0.47
    quantile_embedding.weight   0.52 (tiles: 1.3e-6 of 2.6e-6)           | 0.52
    quantile_embedding.bias     0.52 (wide: 3.0e-6 of 5.8e-6)            | 0.45
    value_net.0.weight          0.56 (tiles)                             | 0.56
    value_net.0.bias            0.47 (wide: 4.4e-6 of 9.4e-6)            | 0.38
    value_net.2.weight          0.57 (fractions)                         | 0.51
    value_net.2.bias            0.55 (ragged A = 63: 1.2e-6 of 2.2e-6)   | 0.36
(`wide` has the widest bars: at E = 128 fp32 rounds the cosine's argument pi * i * tau, up to 402, to 2.4e-5, which the
control and the kernels share; tests/test_iqn_cases.py caps what a case may ask for.)  The grid found no wrong result:
every case, H % 4 != 0 and the three limits included, is inside its bar with a NaN-filled workspace.

Hand mutations of csrc/iqn.hpp these tests were run against on an MI355X, with tests/test_iqn_gpu.py and
tests/test_iqn_online_gpu.py beside them (`old`: the cases those two files had before this grid):
  * `s > 0.f` dropped in iqn_hadamard_bwd_relu_kernel: all 26 learn cases fail; old: the reference golden and the four
    whole-step oracle cases see it too.
  * `r0 + r <= rows` in iqn_embed_wgrad_kernel's staging: all 26 learn cases fail (quantile_embedding's gradient); old: two
    of the four whole-step cases.
  * its bias gradient stored from every blockIdx.y: nothing fails, and nothing can: every blockIdx.y stages the same
    gradient rows and adds them in the same order, so the extra stores carry the same bits.  The guard saves stores only.
  * the head's Bellman-target loop cut to one pass: both `fractions` cases fail, and the head bit test at N'' = 65, 129 and
    256 (tests/test_iqn_online_gpu.py's new shapes); old: nothing.
  * natural k order in iqn_mix_kernel: only the mix bit test fails, at every shape; no oracle comparison moves.
  * the bias dropped where iqn_act_head_kernel runs its scalar branch: every H = 30 act case with A > 1 and both NaN
    probes at H = 30 fail; old: nothing (every old act case has H % 4 == 0).
  * a plain `>` for the act argmax's NaN rule: all eight NaN probes fail; old: nothing.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import iqn_cases as IC
from oracle import iqn_oracle as IO
from porl_amd import engine as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLOOR, CONTROL_FACTOR = 2e-6, 2.0
SENTINEL = -7.25
BUFFERS = ("params", "params_tgt", "grads", "adam_m", "adam_v")
REPLAY = ("states", "actions", "rewards", "next_states", "dones")


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(inputs, fp64 step, the fp32 control's errors) of a learn case: computed once, shared, never modified."""
    d = IC.make_learn(IC.LEARN_CASES[name])
    r64 = IC.step64(d)
    return d, r64, IC.learn_errors(r64, IC.step32(d))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class _Layout:
    def __init__(self, S, H, Ed, A):
        self.shapes = IC.shapes_of(S, H, Ed, A)
        self.offsets, self.n = IC.offsets_of(S, H, Ed, A)
        self.cover = np.zeros(self.n, dtype=bool)
        for off, shp in zip(self.offsets, self.shapes):
            self.cover[off:off + int(np.prod(shp))] = True

    def write(self, flat, tensors):
        """Tensors (a dict under IO.NAMES) into a flat device buffer; the padding is not touched."""
        for name, off, shp in zip(IO.NAMES, self.offsets, self.shapes):
            t = _dev(np.asarray(tensors[name], dtype=np.float32))
            assert tuple(t.shape) == tuple(shp)
            flat[off:off + t.numel()].copy_(t.reshape(-1))

    def tensors(self, flat_host):
        return [flat_host[off:off + int(np.prod(shp))].reshape(shp).copy() for off, shp in zip(self.offsets, self.shapes)]


def _engine(S, A, Ed, H, max_batch, max_tau):
    eng = E.IqnEngine(S, A, Ed, H, max_batch, max_tau, DEV)
    lay = _Layout(S, H, Ed, A)
    assert eng.offsets == lay.offsets and eng.n_params == lay.n
    bufs = {k: torch.zeros(lay.n, dtype=torch.float32, device=DEV) for k in BUFFERS}
    eng.bind(*[bufs[k] for k in BUFFERS])
    return eng, lay, bufs


def _poison(eng):
    """A kernel that reads a workspace column nobody wrote then shows up as a non-finite result, not as luck."""
    eng.workspace.fill_(float("nan"))


def _host(bufs):
    return {k: v.cpu().numpy().copy() for k, v in bufs.items()}


def _run_engine(d):
    """One eng.learn of the case -> (everything the step left, on the host; the engine, its layout and buffers)."""
    c = d["case"]
    eng, lay, bufs = _engine(c["S"], c["A"], c["E"], c["H"], c["B"], max(c["NP"], c["NPP"]))
    for k, src in (("params", d["online"]), ("params_tgt", d["target"]), ("adam_m", d["adam_m"]), ("adam_v", d["adam_v"])):
        lay.write(bufs[k], src)
    lay.write(bufs["grads"], {n: np.full(s, SENTINEL, dtype=np.float32) for n, s in zip(IO.NAMES, lay.shapes)})
    before = _host(bufs)
    args = [_dev(d[k]) for k in REPLAY] + [_dev(d["idx"]), _dev(d["taus_prime"]), _dev(d["taus_dprime"])]
    keep = [a.clone() for a in args]
    _poison(eng)
    hp = eng.hyper(IC.GAMMA, c["kappa"], d["max_norm"], IC.STEP, IC.LR, IC.BETAS, IC.EPS)
    assert eng.learn(hp, *args) == c["B"]
    torch.cuda.synchronize()
    for a, k in zip(args, keep):
        assert torch.equal(a, k), "the step wrote to its inputs"
    out = _host(bufs)
    out["stats"] = eng.stats[:3].cpu().numpy().copy()
    out["before"] = before
    return out, eng, lay, bufs


def _run_autograd(d):
    """The same step through IQNTrainer.learn_on, loaded with the case's parameters, moments and step number."""
    from porl_amd.train.iqn_trainer import IQNTrainer
    c, idx = d["case"], d["idx"]
    t = IQNTrainer(c["S"], c["A"], gamma=IC.GAMMA, device=DEV, learning_rate=IC.LR, batch_size=c["B"], kappa=c["kappa"],
                   embedding_dim=c["E"], hidden_size=c["H"], num_quantiles_n_prime_loss=c["NP"],
                   num_quantiles_n_double_prime_loss=c["NPP"], max_norm=d["max_norm"], buffer_size=8)
    lay = _Layout(c["S"], c["H"], c["E"], c["A"])
    o = t.optimizer
    assert [n for n, _ in t.q_network.named_parameters()] == IO.NAMES and o.flat.numel() == lay.n
    bufs = dict(params=o.flat, params_tgt=t._target.flat, grads=o.grad, adam_m=o.exp_avg, adam_v=o.exp_avg_sq)
    for k, src in (("params", d["online"]), ("params_tgt", d["target"]), ("adam_m", d["adam_m"]), ("adam_v", d["adam_v"])):
        lay.write(bufs[k], src)
    o.step_count = IC.STEP - 1
    before = _host(bufs)
    loss = t.learn_on(*(torch.from_numpy(d[k][idx]) for k in REPLAY), taus_prime=torch.from_numpy(d["taus_prime"]),
                      taus_double_prime=torch.from_numpy(d["taus_dprime"]))
    torch.cuda.synchronize()
    assert o.step_count == IC.STEP
    out = _host(bufs)
    out["stats"] = np.array([loss, float(o._clip[0]), float(o._clip[1])], dtype=np.float32)
    out["before"] = before
    return out, lay


def _check_step(d, r64, control, out, lay):
    """-> [(quantity, error, bar)] of one step; raises on everything that is exact or held at fp32 rounding."""
    c = d["case"]
    assert np.isfinite(out["stats"]).all(), f"non-finite statistics {out['stats']}"
    for k in ("grads", "params", "adam_m", "adam_v"):
        assert np.isfinite(out[k]).all(), f"{k}: non-finite entries"
    assert not (out["grads"][lay.cover] == SENTINEL).any(), "a gradient element was never written"
    got = dict(loss=out["stats"][0], norm=out["stats"][1], coef=out["stats"][2], grads=lay.tensors(out["grads"]))
    err = IC.learn_errors(r64, got)
    bar = lambda x: max(FLOOR, CONTROL_FACTOR * x)
    rows = [(k, err[k], bar(control[k])) for k in IC.STAT_NAMES]
    rows += [("grad " + n, e, bar(x)) for n, e, x in zip(IO.NAMES, err["grads"], control["grads"])]
    if not c["clip"]:
        assert out["stats"][2] == 1.0
    # Adam on the device's OWN gradient buffer, over the whole flat image (padding included: it stays zero)
    b = out["before"]
    p, m, v = IC.adam64(b["params"], out["grads"], b["adam_m"], b["adam_v"])
    np.testing.assert_allclose(out["params"], p, atol=1e-7, rtol=1e-6, err_msg="params after Adam")
    np.testing.assert_allclose(out["adam_m"], m, atol=1e-9, rtol=1e-5, err_msg="adam_m")
    np.testing.assert_allclose(out["adam_v"], v, atol=1e-12, rtol=1e-5, err_msg="adam_v")
    assert (out["params"][lay.cover] != b["params"][lay.cover]).mean() > 0.5          # the step did step
    for k in ("params", "grads", "adam_m", "adam_v"):
        assert not out[k][~lay.cover].any(), f"{k}: non-zero padding between tensors"
    assert out["params_tgt"].tobytes() == b["params_tgt"].tobytes(), "params_tgt changed"
    return rows


def _report(tag, name, rows):
    worst = max(rows, key=lambda r: r[1] / r[2])
    print()
    for what, e, bar in rows:
        print(f"[iqn-engine] {tag} {name} | {what} | err {e:.3g} bar {bar:.3g} ratio {e / bar:.3f}")
    failed = [f"{what}: error {e:.3g} > bar {bar:.3g}" for what, e, bar in rows if not e <= bar]
    assert not failed, f"{name}: {len(failed)} quantities past their bar (worst {worst[0]}):\n" + "\n".join(failed)


@pytest.mark.parametrize("name", IC.LEARN_NAMES)
def test_learn_matches_the_fp64_oracle(name):
    d, r64, control = _ref(name)
    out, eng, lay, bufs = _run_engine(d)
    rows = _check_step(d, r64, control, out, lay)
    _report("engine", name, rows)


@pytest.mark.parametrize("name", [n for n, c in IC.LEARN_CASES.items() if c["shape"] in ("one", "ragged", "tiles") and c["A"] ==
                                  IC.LEARN_SHAPES[c["shape"]][3] and c["kappa"] == 1.0])
def test_autograd_path_meets_the_same_bars(name):
    d, r64, control = _ref(name)
    out, lay = _run_autograd(d)
    rows = _check_step(d, r64, control, out, lay)
    _report("autograd", name, rows)


def test_act_record_carries_the_statistics_of_the_learn_step_before_it():
    """n_stats = 3 after a learn step: words 8..10 of the record are stats[0:3] bit for bit, and the action is the oracle's
    on the parameters the step left."""
    d, _, _ = _ref("ragged-a5-k1.0-free")
    c = d["case"]
    out, eng, lay, bufs = _run_engine(d)
    P = dict(zip(IO.NAMES, lay.tensors(out["params"])))
    taus = np.random.default_rng(7).random((d["n_rows"], 3)).astype(np.float32)
    q = IC.mean_q(P, d["states"], taus)
    row = int(np.flatnonzero(IC.top2_gap(q) >= IC.ACT_MIN_GAP)[0])
    rec = torch.full((2, 16), -1, dtype=torch.int32, device=DEV)
    eng.act(rec[0], _dev(taus[row:row + 1]), inline=d["states"][row], n_stats=3)
    eng.act(rec[1], _dev(taus[row:row + 1]), states=_dev(d["states"]), row=row, n_stats=2)
    torch.cuda.synchronize()
    rec = rec.cpu().numpy()
    assert rec[0, 0] == rec[1, 0] == int(q[row].argmax())
    assert rec[0, 8:11].tobytes() == out["stats"].tobytes() and rec[1, 8:10].tobytes() == out["stats"][:2].tobytes()
    assert (rec[0, 1:8] == -1).all() and (rec[0, 11:] == -1).all() and (rec[1, 10:] == -1).all()


ACT_IDS = [("grid",) + k for k in IC.ACT_GRID] + [("probe",) + k for k in IC.ACT_PROBES]


@pytest.mark.parametrize("key", ACT_IDS, ids=lambda k: "-".join(map(str, k)))
def test_act_answers_with_the_oracles_action(key):
    c = IC.act_grid_case(*key[1:]) if key[0] == "grid" else IC.act_probe_case(*key[1:])
    H, n_tau = (key[1], key[2]) if key[0] == "grid" else (key[2], key[3])
    A = c["P"]["value_net.2.bias"].shape[0]
    eng, lay, bufs = _engine(IC.ACT2_S, A, IC.ACT2_E, H, 1, n_tau)
    lay.write(bufs["params"], c["P"])
    if c["which"]:
        lay.write(bufs["params_tgt"], c["T"])
    else:
        bufs["params_tgt"].fill_(float("nan"))            # which = 0 reads nothing of the target parameters
    _poison(eng)                                          # before the first act
    n = len(c["states"])
    states, taus = _dev(c["states"]), _dev(c["taus"])
    rec = torch.full((2 * n, 16), -1, dtype=torch.int32, device=DEV)
    for i in range(n):
        eng.act(rec[i], taus[i:i + 1], inline=c["states"][i], which=c["which"], n_stats=0)
        eng.act(rec[n + i], taus[i:i + 1], states=states, row=i, which=c["which"], n_stats=0)
    torch.cuda.synchronize()
    rec = rec.cpu().numpy()
    np.testing.assert_array_equal(rec[:n, 0], c["want"], err_msg="inline state")
    np.testing.assert_array_equal(rec[n:, 0], c["want"], err_msg="device row")
    assert (rec[:, 1:] == -1).all()                       # n_stats = 0: the action word only
