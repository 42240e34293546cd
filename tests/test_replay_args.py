"""engine.replay_args, the one check of device-resident replay arrays in front of every row-sourced native call, on CPU
tensors (it makes no native call, so it needs neither a GPU nor an engine): what it refuses, naming the array, and the
argument tuple it hands to the C ABI."""
import pytest
import torch

from porl_amd.engine import replay_args

CPU = torch.device("cpu")
S, ROWS = 6, 10
NAMES = ("states", "actions", "rewards", "next_states", "dones")


def _arrays():
    return dict(states=torch.zeros(ROWS, S), actions=torch.zeros(ROWS, dtype=torch.int64), rewards=torch.zeros(ROWS),
                next_states=torch.zeros(ROWS, S), dones=torch.zeros(ROWS))


def _call(a, **kw):
    return replay_args(*[a[k] for k in NAMES], kw.pop("state_dim", S), CPU, **kw)


def _strided(x):
    """The same values behind a stride of two elements."""
    wide = torch.zeros(*x.shape[:-1], 2 * x.shape[-1], dtype=x.dtype) if x.dim() > 1 else torch.zeros(2 * x.shape[0], dtype=x.dtype)
    return wide[..., ::2]


@pytest.mark.parametrize("fault", ["dtype", "device", "stride"])
@pytest.mark.parametrize("name", NAMES)
def test_each_array_is_refused_by_name(name, fault):
    a = _arrays()
    x = a[name]
    if fault == "dtype":
        a[name] = x.to(torch.float64 if x.dtype == torch.float32 else torch.int32)
    elif fault == "device":
        a[name] = torch.empty(x.shape, dtype=x.dtype, device="meta")
    else:
        a[name] = _strided(x)
        assert not a[name].is_contiguous() and a[name].shape == x.shape
    with pytest.raises(RuntimeError, match=rf"^{name}:"):
        _call(a)


def test_shapes_rows_and_indices_are_refused_by_name():
    a = _arrays()
    with pytest.raises(RuntimeError, match=r"^states:.*state_dim is 7"):
        _call(a, state_dim=S + 1)
    b = dict(a, next_states=torch.zeros(ROWS - 1, S))
    with pytest.raises(RuntimeError, match=r"^next_states:"):
        _call(b)
    for name in NAMES:                                     # one array shorter than the rows the sampler may draw from
        b = dict(a)
        b[name] = a[name][:ROWS - 1].contiguous()
        with pytest.raises(RuntimeError, match=rf"^{name}:.*{ROWS} rows"):
            _call(b, n_rows=ROWS)
    _call(a, n_rows=ROWS)
    for idx, why in ((torch.zeros(4, dtype=torch.int32), "dtype"), (torch.zeros(8, dtype=torch.int64)[::2], "stride"),
                     (torch.empty(4, dtype=torch.int64, device="meta"), "device")):
        with pytest.raises(RuntimeError, match=r"^idx:"):
            _call(a, idx=idx)


def test_a_valid_set_comes_back_in_abi_order():
    a = _arrays()
    a["states"] = a["states"].view(ROWS, 2, 3)             # rows of any shape whose size is state_dim
    a["next_states"] = a["next_states"].view(ROWS, 2, 3)
    for kw in ({}, dict(n_rows=ROWS), dict(idx=torch.arange(4)), dict(n_rows=3, idx=torch.arange(4))):
        out = _call(a, **kw)
        assert len(out) == 7 and out[1] == S and out[5] == S
        assert [p.value for p in out[:1] + out[2:5] + out[6:]] == \
            [a[k].data_ptr() for k in ("states", "actions", "rewards", "next_states", "dones")]
