"""Writes tests/golden/qnet_layout.json: what the Q-network engine's host planner (porl_qnet_create) makes of a list of
network shapes.

    python tests/helpers/gen_qnet_layout.py

Needs the built library and no GPU: creating a handle and asking it for its layout launches nothing.  Run at the commit
whose planner is the yardstick (the fixture was written before the planner's LDS arithmetic was gathered into one
function); tests/test_qnet_layout.py compares the current build with it.  Kernel selection is the process default.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(os.path.dirname(HERE), "golden", "qnet_layout.json")

# (state_dim, hidden widths, n_actions, max_batch): every branch of the planner from both sides
SHAPES = [
    (60, (64, 128, 64), 10, 4096),              # the flagship CQL network: both step kernels fit
    (7, (64, 64), 5, 40),                       # state_dim % 16 != 0, n_actions % 32 != 0, max_batch % 16 != 0
    (7, (64, 64), 5, 1),
    (60, (128,), 10, 256),                      # widest hidden layer the one-launch kernel takes ...
    (60, (129,), 10, 256),                      # ... and one more
    (128, (64,), 4, 64),                        # the same for the input ...
    (129, (64,), 4, 64),
    (16, (64,), 128, 64),                       # ... and for the output
    (16, (64,), 129, 64),
    (8, (32, 32, 32, 32), 4, 33),               # QF_MAX_LIN Linear layers ...
    (8, (32, 32, 32, 32, 32), 4, 33),           # ... and QF_MAX_LIN + 1
    (60, (128, 128), 10, 100),                  # one weight image fits beside the activations, two do not
    (128, (128, 128, 128, 128), 128, 64),       # every width and the depth allowed, but over the LDS byte budget
    (48, (200, 160), 6, 256),                   # wide: the multi-launch path
    (9, (64, 64), 60, 128),                     # a distributional head's A x N outputs, still <= 128
    (9, (64, 64), 255, 128),                    # ... and beyond
    (17, (33, 31, 65, 1, 96, 15, 100, 12), 3, 50),      # PORL_MAX_HIDDEN hidden layers of odd widths
    (10, (1024,), 6, 8),                        # widest layer the one-workgroup act kernel takes ...
    (10, (1025,), 6, 8),                        # ... and one more
    (1000, (520,), 6, 8),                       # narrow enough for it, but over 2^19 parameter floats
    (4, (8,), 4096, 2),                         # the most outputs an engine accepts
]


def describe(lib, N, shape):
    S, hidden, A, B = shape
    cfg = N.QnetCfg()
    cfg.state_dim, cfg.n_actions, cfg.n_hidden, cfg.max_batch = S, A, len(hidden), B
    for i, w in enumerate(hidden):
        cfg.hidden[i] = w
    h = C.c_void_p()
    N.check(lib.porl_qnet_create(C.byref(cfg), C.byref(h)), "porl_qnet_create")
    try:
        off, r, c, ld = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        tensors = []
        for i in range(int(lib.porl_qnet_tensors(h))):
            N.check(lib.porl_qnet_tensor_info(h, i, C.byref(off), C.byref(r), C.byref(c), C.byref(ld)), "porl_qnet_tensor_info")
            tensors.append([off.value, r.value, c.value, ld.value])
        return {"state_dim": S, "hidden": list(hidden), "n_actions": A, "max_batch": B,
                "param_floats": int(lib.porl_qnet_param_floats(h)),
                "workspace_floats": int(lib.porl_qnet_workspace_floats(h)),
                "one_launch": int(lib.porl_qnet_one_launch(h)),
                "can_sample": int(lib.porl_qnet_can_sample(h)),
                "act_ok": int(lib.porl_qnet_act_ok(h)),
                "tensors": tensors}
    finally:
        lib.porl_qnet_destroy(h)


def layouts():
    from porl_amd import _native as N
    lib = N.lib()
    return [describe(lib, N, s) for s in SHAPES]


if __name__ == "__main__":
    rows = layouts()
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    for r in rows:
        print(r["state_dim"], r["hidden"], r["n_actions"], r["max_batch"], "->", r["param_floats"], r["workspace_floats"],
              r["one_launch"], r["can_sample"], r["act_ok"])
    print(f"{len(rows)} shapes -> {OUT}")
