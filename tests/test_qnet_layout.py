"""The Q-network engine's host planner (porl_qnet_create, csrc/qnet_api.inc) against tests/golden/qnet_layout.json, the
record of what it planned before its LDS arithmetic was gathered into one function (tests/helpers/gen_qnet_layout.py).
No GPU: creating a handle and asking for its layout launches nothing."""
import json
import os

import pytest

from conftest import GOLDEN
from helpers import gen_qnet_layout as G

with open(os.path.join(GOLDEN, "qnet_layout.json")) as _f:
    WANT = json.load(_f)

QF_MAX_LIN, QF_MAX_W = 5, 128          # csrc/qnet_fused.hpp


def _key(r):
    return (r["state_dim"], tuple(r["hidden"]), r["n_actions"], r["max_batch"])


def test_fixture_straddles_every_branch_of_the_planner():
    """The shapes, judged by what the fixture recorded for them.

    LDS budget of the step kernel (qnet_fused.hpp): 160 KiB - 1 KiB = 40704 floats.  One block holds 32 rows of every
    layer's activation at round32(width) + 4 floats, two ping-pong buffers of the widest, and one weight image + bias
    row; the two-group kernel (in-kernel sampling needs it) holds a second image.  60-128-128-10:
    32 * (68 + 132 + 132 + 36) + 2 * 32 * 132 + 128 * 133 = 37248 <= 40704 < 37248 + 17024, so a shape with
    one_launch == 1 and can_sample == 0 exists, and the fixture has it."""
    by = {_key(r): r for r in WANT}
    assert len(by) == len(WANT) == len(G.SHAPES) and set(by) == {(s, tuple(h), a, b) for s, h, a, b in G.SHAPES}

    def flags(*k):
        return by[k]["one_launch"], by[k]["can_sample"]
    # width 128 against 129: hidden, input and output layer
    assert flags(60, (128,), 10, 256)[0] == 1 and flags(60, (129,), 10, 256)[0] == 0
    assert flags(128, (64,), 4, 64)[0] == 1 and flags(129, (64,), 4, 64)[0] == 0
    assert flags(16, (64,), 128, 64)[0] == 1 and flags(16, (64,), 129, 64)[0] == 0
    # QF_MAX_LIN against QF_MAX_LIN + 1 Linear layers
    assert flags(8, (32,) * (QF_MAX_LIN - 1), 4, 33) == (1, 1) and flags(8, (32,) * QF_MAX_LIN, 4, 33) == (0, 0)
    # the one-group plan fits, the two-group plan does not
    assert flags(60, (128, 128), 10, 100) == (1, 0)
    # width and depth allowed, the byte budget alone says no
    k = (128, (128,) * (QF_MAX_LIN - 1), 128, 64)
    assert max(k[0], k[2], *k[1]) <= QF_MAX_W and len(k[1]) + 1 <= QF_MAX_LIN and flags(*k) == (0, 0)
    assert any(r["state_dim"] % 16 and r["n_actions"] % 32 and r["max_batch"] % 16 and r["one_launch"] for r in WANT)
    # the act kernel's two bounds, each alone
    assert by[(10, (1024,), 6, 8)]["act_ok"] == 1 and by[(10, (1025,), 6, 8)]["act_ok"] == 0
    assert by[(1000, (520,), 6, 8)]["act_ok"] == 0 and by[(1000, (520,), 6, 8)]["param_floats"] > 1 << 19
    for r in WANT:
        assert len(r["tensors"]) == 2 * (len(r["hidden"]) + 1)


@pytest.fixture(scope="module")
def got():
    return {_key(r): r for r in G.layouts()}


@pytest.mark.parametrize("want", WANT, ids=lambda r: "-".join(map(str, (r["state_dim"], *r["hidden"], r["n_actions"], "b%d" % r["max_batch"]))))
def test_planner_matches_the_recorded_layout(got, want):
    have = got[_key(want)]
    for field in ("param_floats", "workspace_floats", "one_launch", "can_sample", "act_ok"):
        assert have[field] == want[field], field
    assert have["tensors"] == want["tensors"]
