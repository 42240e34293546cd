"""Writes tests/golden/episodes_ref.npz: what the reference's trajectory-level dataset functions return.

    python tests/helpers/gen_episodes_golden.py [reference_dir]

Runs on a CPU box with the reference checked out (default /root/reference); never on the GPU machine.  For every vector
of tests/helpers/episode_cases.py:golden_vectors it records `extract_done_makers(dones)` and
`return_range({'rewards', 'terminals'}, cap)` for the caps of episode_cases.CAPS, and for every entry of
episode_cases.PAIR_CASES the (choice, rand, rand) stream `_sample_indces` consumes under a pinned np.random.seed,
re-drawn in the reference's order, beside the function's own result under the same seed.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import episode_cases as EC  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(HERE), "golden", "episodes_ref.npz")


def main():
    sys.path.insert(0, REF)
    from util import util as U
    vecs = EC.golden_vectors()
    z = {}
    for name, (rew, dones) in vecs.items():
        assert rew.dtype == np.float32 and dones.dtype == np.float32 and rew.size == dones.size <= 5000
        starts, ends, lengths = U.extract_done_makers(dones)
        assert ends.size >= 1
        z[f"{name}_rewards"], z[f"{name}_dones"] = rew, dones
        z[f"{name}_starts"], z[f"{name}_ends"], z[f"{name}_lengths"] = (np.asarray(a, dtype=np.int64) for a in (starts, ends, lengths))
        ds = {"rewards": torch.from_numpy(rew), "terminals": torch.from_numpy(dones)}
        z[f"{name}_range"] = np.array([U.return_range(ds, cap) for cap in EC.CAPS], dtype=np.float64)
        print(f"{name:12s} N={rew.size:5d} E={ends.size:5d} range@1000={z[f'{name}_range'][-1]}")
    for case, vec, seed, batch, terminals_from in EC.PAIR_CASES:
        flags = vecs[vec][1]
        if terminals_from is None:
            ds = {"terminals": torch.from_numpy(flags)}
        else:
            other = vecs[terminals_from][1]
            assert other.size == flags.size
            ds = {"terminals": torch.from_numpy(other), "timeouts": torch.from_numpy(flags)}
        n_traj = int(np.count_nonzero(flags != 0))
        np.random.seed(seed)
        traj = np.random.choice(n_traj, batch)
        u1 = np.random.rand(batch)
        u2 = np.random.rand(batch)
        np.random.seed(seed)
        start, goal = U._sample_indces(ds, batch)
        z[f"pairs_{case}_traj"], z[f"pairs_{case}_u1"], z[f"pairs_{case}_u2"] = traj.astype(np.int64), u1, u2
        z[f"pairs_{case}_start"], z[f"pairs_{case}_goal"] = start.astype(np.int64), goal.astype(np.int64)
        print(f"pairs {case}: E={n_traj} B={batch}")
    np.savez_compressed(OUT, **z)
    print(f"-> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
