"""Which labelled launches the IQL engine's entry points issue (csrc/iql_api.inc), case by case, against
tests/golden/iql_launches.json — recorded by tests/helpers/gen_iql_launches.py before the engine's host code was gathered
into one copy of each step.  The comparison is exact: the calls in order, and for each call every profile label (phase
prefix and tile included) with its launch count.  The forward paths' arithmetic is pinned by test_forward_gpu.py, the
updates' by the oracle tests; this file pins the HOST side — which kernel, which tile, which phase, how often.  GPU only.
"""
import json

import pytest

from helpers import gen_iql_launches as G

pytestmark = pytest.mark.gpu

with open(G.OUT) as f:
    GOLDEN = json.load(f)


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_the_entry_points_issue_the_recorded_launches(name):
    case = next(c for c in G.CASES if c.name == name)
    got = G.record(case)
    want = GOLDEN[name]
    assert [call for call, _ in got] == [call for call, _ in want]
    for (call, labels), (_, expected) in zip(got, want):
        assert labels == expected, (name, call)
