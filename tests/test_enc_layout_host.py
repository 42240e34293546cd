"""The encoder engine's buffer layout (porl_enc_create, no device needed) against integers recorded from the library
before the forward was split into named steps (commit 64fc13e): parameter, statistic and workspace sizes, the tap
offsets and every tensor offset, for the seven configurations of tests/helpers/encoder_fp32_cases.py and the reference
architecture in each of the three bf16_operands modes.  The packed weight images live in the workspace, so a size
function that drifts from the expression it replaced moves these numbers."""
import ctypes as C

import pytest

from helpers import encoder_fp32_cases as EC
from porl_amd import _native as N

# name -> (n_ang, n_dist, embed, depth0, depth1, n_div, max_batch, mlp_ratio, bf16_operands)
CONFIGS = {c.name: (c.ab, c.db, c.embed, c.depths[0], c.depths[1], c.n_div, c.B, c.mlp_ratio, 0) for c in EC.CASES}
CONFIGS.update({f"ref-360x256-b512-bf16_operands={m}": (360, 256, 96, 1, 2, 4, 512, 2.0, m) for m in (0, 1, 2)})

# (param floats, stat floats, workspace floats, the four tap offsets, every tensor offset in index order), printed by
# `python tests/test_enc_layout_host.py` at commit 64fc13e
REF_TENSORS = (0, 4608, 4704, 4800, 23232, 23424, 23616, 42048, 47232, 120960, 121152, 121344, 195072, 195456, 195840, 269568,
               290304, 364032, 364416, 364800, 438528, 459264, 705024, 1032704)
REF_TAPS = (141557760, 1911029760, 2052587520, 2052685824)
RECORDED = {
    '40x64-b3': (1032960, 2496, 3730692, (23040, 311040, 334080, 334656), REF_TENSORS),
    '84x84-b5': (1032960, 2496, 4944364, (105840, 1428840, 1524840, 1525800), REF_TENSORS),
    '360x256-b2': (1032960, 2496, 11545156, (552960, 7464960, 8017920, 8018304), REF_TENSORS),
    '360x256-b7': (1032960, 2496, 31944836, (1935360, 26127360, 28062720, 28064064), REF_TENSORS),
    '40x64-e64-d21-b2': (641152, 1408, 2342404, (15360, 143360, 153600, 153856),
                         (0, 3072, 3136, 3200, 11392, 11520, 11648, 19840, 22144, 30336, 30464, 30592, 38784, 41088, 73856,
                          73984, 74112, 106880, 107136, 107392, 140160, 149376, 313216, 640896)),
    '40x64-e32-d11-r3-b2': (462592, 768, 1745796, (15360, 112640, 117760, 117888),
                            (0, 1536, 1568, 1600, 4672, 4768, 4864, 7936, 10240, 18432, 18496, 18560, 30848, 31040, 31232,
                             43520, 52736, 134656, 462336)),
    '40x64-e32-d11-r2.25-b2': (454768, 624, 1344180, (15360, 104960, 110080, 110208),
                               (0, 1536, 1568, 1600, 3904, 3976, 4048, 6352, 8656, 16848, 16912, 16976, 26192, 26336, 26480,
                                35696, 44912, 126832, 454512)),
    'ref-360x256-b512-bf16_operands=0': (1032960, 2496, 2092312516, REF_TAPS, REF_TENSORS),
    'ref-360x256-b512-bf16_operands=1': (1032960, 2496, 2092312516, REF_TAPS, REF_TENSORS),
    'ref-360x256-b512-bf16_operands=2': (1032960, 2496, 2092553284, REF_TAPS, REF_TENSORS),
}


def layout(cfg):
    ab, db, embed, d0, d1, n_div, B, ratio, mode = cfg
    lib = N.lib()
    c = N.EncCfg(ab, db, embed, d0, d1, n_div, 1280, 256, B, ratio, 1e-5, 0.1, mode)
    h = C.c_void_p()
    N.check(lib.porl_enc_create(C.byref(c), C.byref(h)), "porl_enc_create")
    try:
        off, rps, cols, eb = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        taps, tensors = [], []
        for i in range(4):
            N.check(lib.porl_enc_tap_info(h, i, C.byref(off), C.byref(rps), C.byref(cols), C.byref(eb)))
            taps.append(off.value)
        for i in range(int(lib.porl_enc_tensors(h))):
            N.check(lib.porl_enc_tensor_info(h, i, C.byref(off), None, None, 0))
            tensors.append(off.value)
        return (int(lib.porl_enc_param_floats(h)), int(lib.porl_enc_stat_floats(h)), int(lib.porl_enc_workspace_floats(h)),
                tuple(taps), tuple(tensors))
    finally:
        lib.porl_enc_destroy(h)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_layout_equals_the_recorded_integers(name):
    got = layout(CONFIGS[name])
    assert got == RECORDED[name], (got, RECORDED[name])


if __name__ == "__main__":
    for name, cfg in CONFIGS.items():
        print(f"    {name!r}: {layout(cfg)!r},")
