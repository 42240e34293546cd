"""tests/golden/iql_launches.json against the case list of tests/helpers/gen_iql_launches.py (no GPU): the fixture names
exactly the listed cases, every case records a call, and the list still spans what it is there for."""
import json

from helpers import gen_iql_launches as G


def _golden():
    with open(G.OUT) as f:
        return json.load(f)


def test_the_fixture_names_exactly_the_listed_cases():
    names = [c.name for c in G.CASES]
    assert len(set(names)) == len(names)
    golden = _golden()
    assert sorted(golden) == sorted(names)
    for name, calls in golden.items():
        assert calls and all(isinstance(call, str) and isinstance(labels, list) for call, labels in calls), name
        assert len(calls) % G.UPDATES == 0, name


def test_the_cases_span_shapes_patterns_and_selection_keys():
    assert {c.shape for c in G.CASES} == set(G.SHAPES)
    assert {c.pattern for c in G.CASES} == set(G.PATTERNS)
    assert all(c.covers for c in G.CASES)
    keys = {k for c in G.CASES for k, _ in c.tune}
    assert {"skinny", "l0_kernel", "iql_fold", "skinny_pipelined", "vbwd_tile_short", "l0_tile"} <= keys
    modes = {c.mode for c in G.CASES}
    assert {0, G.TWO_SLOTS, G.FOLD_COMBINE, G.SHORT_BLOCKS, G.PIPE} <= modes


def test_the_fixture_reaches_every_labelled_kernel_of_the_engine():
    labels = {label.split(":")[-1].split(".")[-1].split("<")[0] for calls in _golden().values() for _, ls in calls for label, _ in ls}
    assert labels == {"gemm_f32_kernel", "l0_fwd_kernel", "small_fwd_kernel", "mean_skinny_kernel", "wgrad_skinny_kernel",
                      "out_bwd_kernel", "relu_head_bwd_kernel", "policy_nll_kernel", "policy_weight_kernel",
                      "multi_reduce_kernel", "adam_ema_kernel", "sampled_batch_kernel", "indexed_batch_kernel"}
