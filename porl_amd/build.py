"""Build libporl_hip.so for gfx950 in-tree:  python -m porl_amd.build

hipcc cross-compiles without a GPU.  The .so is git-ignored but travels with the gpurun snapshot.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "porl_api.hip")
DEPS = sorted(os.path.join(HERE, "csrc", f) for f in os.listdir(os.path.join(HERE, "csrc"))) + \
       [os.path.join(os.path.dirname(HERE), "include", "porl_hip.h")]
OUT = os.path.join(HERE, "lib", "libporl_hip.so")


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


HASH = OUT + ".srchash"


def source_hash():
    """sha256 over the library's sources (csrc/* and the header), in name order."""
    import hashlib
    h = hashlib.sha256()
    for d in DEPS:
        h.update(os.path.basename(d).encode() + b"\0")
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def up_to_date():
    """The binary is git-ignored and travels by snapshot, so staleness is decided by CONTENT: the hash of the sources it
    was built from is kept beside it (modification times do not survive a snapshot reliably)."""
    try:
        return os.path.exists(OUT) and open(HASH).read().strip() == source_hash()
    except OSError:
        return False


def build(force=False, verbose=True):
    sh = source_hash()
    if not force and up_to_date():
        if verbose:
            print(f"libporl_hip.so is current (sources sha256 {sh[:16]})", flush=True)
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-o", OUT, SRC]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    with open(HASH, "w") as f:
        f.write(sh + "\n")
    if verbose:
        print(f"built from sources sha256 {sh[:16]}", flush=True)
    return OUT


SAN_OUT = os.path.join(HERE, "lib", "libporl_hip_host_san.so")
SAN_DRIVER_SRC = os.path.join(os.path.dirname(HERE), "tests", "helpers", "abi_reject.cpp")
SAN_DRIVER = os.path.join(HERE, "lib", "abi_reject_san")
# second driver, same library: the entry points that read a packed replay store in place (tests/test_enc_replay_host.py)
SAN_ROWS_DRIVER_SRC = os.path.join(os.path.dirname(HERE), "tests", "helpers", "abi_reject_rows.cpp")
SAN_ROWS_DRIVER = os.path.join(HERE, "lib", "abi_reject_rows_san")
# third driver: the episode-table / hindsight-pair entry points (tests/test_episodes_host.py)
SAN_EPISODES_DRIVER_SRC = os.path.join(os.path.dirname(HERE), "tests", "helpers", "abi_reject_episodes.cpp")
SAN_EPISODES_DRIVER = os.path.join(HERE, "lib", "abi_reject_episodes_san")
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build_sanitized(force=False, verbose=True):
    """The same translation unit with AddressSanitizer + UBSan on the HOST half (planner, validation, layout code; the
    device half is compiled as usual and never runs), plus the drivers that walk the rejected-argument paths
    (tests/helpers/abi_reject.cpp -> SAN_DRIVER, tests/helpers/abi_reject_rows.cpp -> SAN_ROWS_DRIVER,
    tests/helpers/abi_reject_episodes.cpp -> SAN_EPISODES_DRIVER).  CPU-only check: GPU sanitizers are not available on
    this pool.  Returns SAN_DRIVER; cached by source hash like the product library."""
    import hashlib
    drivers = ((SAN_DRIVER_SRC, SAN_DRIVER), (SAN_ROWS_DRIVER_SRC, SAN_ROWS_DRIVER), (SAN_EPISODES_DRIVER_SRC, SAN_EPISODES_DRIVER))
    h = hashlib.sha256((source_hash() + "".join(open(src).read() for src, _ in drivers)).encode()).hexdigest()
    tag = SAN_OUT + ".srchash"
    try:
        if not force and all(os.path.exists(f) for f in (SAN_OUT, *(out for _, out in drivers))) and open(tag).read().strip() == h:
            return SAN_DRIVER
    except OSError:
        pass
    os.makedirs(os.path.dirname(SAN_OUT), exist_ok=True)
    clangxx = os.path.join(os.path.dirname(os.path.dirname(hipcc())), "lib", "llvm", "bin", "clang++")
    cxx = clangxx if os.path.exists(clangxx) else "clang++"
    cmds = [[hipcc(), "--offload-arch=gfx950", "-fno-gpu-sanitize", *SAN_FLAGS, "-O1", "-std=c++17", "-shared", "-fPIC",
             "-o", SAN_OUT, SRC]]
    cmds += [[cxx, "-std=c++17", "-O1", "-g", *SAN_FLAGS, "-o", out, src, SAN_OUT, "-Wl,-rpath," + os.path.dirname(SAN_OUT)]
             for src, out in drivers]
    for cmd in cmds:
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL if not verbose else None)
    with open(tag, "w") as f:
        f.write(h + "\n")
    return SAN_DRIVER


# fourth driver, built by a function of its own: the row-partition entry points (tests/test_holdout_host.py)
SAN_HOLDOUT_DRIVER_SRC = os.path.join(os.path.dirname(HERE), "tests", "helpers", "abi_reject_holdout.cpp")
SAN_HOLDOUT_DRIVER = os.path.join(HERE, "lib", "abi_reject_holdout_san")


def build_sanitized_holdout(force=False, verbose=True):
    """tests/helpers/abi_reject_holdout.cpp -> SAN_HOLDOUT_DRIVER, a stand-alone program linked against the host-only
    sanitized library of `build_sanitized` (built first when it is not current).  Cached by the hash of the library's
    sources and the driver's.  Returns SAN_HOLDOUT_DRIVER."""
    import hashlib
    build_sanitized(force=force, verbose=verbose)
    h = hashlib.sha256((source_hash() + open(SAN_HOLDOUT_DRIVER_SRC).read()).encode()).hexdigest()
    tag = SAN_HOLDOUT_DRIVER + ".srchash"
    try:
        if not force and os.path.exists(SAN_HOLDOUT_DRIVER) and open(tag).read().strip() == h:
            return SAN_HOLDOUT_DRIVER
    except OSError:
        pass
    clangxx = os.path.join(os.path.dirname(os.path.dirname(hipcc())), "lib", "llvm", "bin", "clang++")
    cmd = [clangxx if os.path.exists(clangxx) else "clang++", "-std=c++17", "-O1", "-g", *SAN_FLAGS, "-o", SAN_HOLDOUT_DRIVER,
           SAN_HOLDOUT_DRIVER_SRC, SAN_OUT, "-Wl,-rpath," + os.path.dirname(SAN_OUT)]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL if not verbose else None)
    with open(tag, "w") as f:
        f.write(h + "\n")
    return SAN_HOLDOUT_DRIVER


# fifth driver, built the same way: the column-statistics / affine entry points (tests/test_normalize_host.py)
SAN_NORMALIZE_DRIVER_SRC = os.path.join(os.path.dirname(HERE), "tests", "helpers", "abi_reject_normalize.cpp")
SAN_NORMALIZE_DRIVER = os.path.join(HERE, "lib", "abi_reject_normalize_san")


def build_sanitized_normalize(force=False, verbose=True):
    """tests/helpers/abi_reject_normalize.cpp -> SAN_NORMALIZE_DRIVER, a stand-alone program linked against the host-only
    sanitized library of `build_sanitized` (built first when it is not current).  Cached by the hash of the library's
    sources and the driver's.  Returns SAN_NORMALIZE_DRIVER."""
    import hashlib
    build_sanitized(force=force, verbose=verbose)
    h = hashlib.sha256((source_hash() + open(SAN_NORMALIZE_DRIVER_SRC).read()).encode()).hexdigest()
    tag = SAN_NORMALIZE_DRIVER + ".srchash"
    try:
        if not force and os.path.exists(SAN_NORMALIZE_DRIVER) and open(tag).read().strip() == h:
            return SAN_NORMALIZE_DRIVER
    except OSError:
        pass
    clangxx = os.path.join(os.path.dirname(os.path.dirname(hipcc())), "lib", "llvm", "bin", "clang++")
    cmd = [clangxx if os.path.exists(clangxx) else "clang++", "-std=c++17", "-O1", "-g", *SAN_FLAGS, "-o", SAN_NORMALIZE_DRIVER,
           SAN_NORMALIZE_DRIVER_SRC, SAN_OUT, "-Wl,-rpath," + os.path.dirname(SAN_OUT)]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL if not verbose else None)
    with open(tag, "w") as f:
        f.write(h + "\n")
    return SAN_NORMALIZE_DRIVER


# sixth driver, built the same way: the goal-conditioned behaviour-cloning entry points (tests/test_goal_bc_host.py)
SAN_GOAL_BC_DRIVER_SRC = os.path.join(os.path.dirname(HERE), "tests", "helpers", "abi_reject_goal_bc.cpp")
SAN_GOAL_BC_DRIVER = os.path.join(HERE, "lib", "abi_reject_goal_bc_san")


def build_sanitized_goal_bc(force=False, verbose=True):
    """tests/helpers/abi_reject_goal_bc.cpp -> SAN_GOAL_BC_DRIVER, a stand-alone program linked against the host-only
    sanitized library of `build_sanitized` (built first when it is not current).  Cached by the hash of the library's
    sources and the driver's.  Returns SAN_GOAL_BC_DRIVER."""
    import hashlib
    build_sanitized(force=force, verbose=verbose)
    h = hashlib.sha256((source_hash() + open(SAN_GOAL_BC_DRIVER_SRC).read()).encode()).hexdigest()
    tag = SAN_GOAL_BC_DRIVER + ".srchash"
    try:
        if not force and os.path.exists(SAN_GOAL_BC_DRIVER) and open(tag).read().strip() == h:
            return SAN_GOAL_BC_DRIVER
    except OSError:
        pass
    clangxx = os.path.join(os.path.dirname(os.path.dirname(hipcc())), "lib", "llvm", "bin", "clang++")
    cmd = [clangxx if os.path.exists(clangxx) else "clang++", "-std=c++17", "-O1", "-g", *SAN_FLAGS, "-o", SAN_GOAL_BC_DRIVER,
           SAN_GOAL_BC_DRIVER_SRC, SAN_OUT, "-Wl,-rpath," + os.path.dirname(SAN_OUT)]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL if not verbose else None)
    with open(tag, "w") as f:
        f.write(h + "\n")
    return SAN_GOAL_BC_DRIVER


# seventh driver, built the same way: the navigation simulator's entry points (tests/test_navsim_host.py)
SAN_NAVSIM_DRIVER_SRC = os.path.join(os.path.dirname(HERE), "tests", "helpers", "abi_reject_navsim.cpp")
SAN_NAVSIM_DRIVER = os.path.join(HERE, "lib", "abi_reject_navsim_san")


def build_sanitized_navsim(force=False, verbose=True):
    """tests/helpers/abi_reject_navsim.cpp -> SAN_NAVSIM_DRIVER, a stand-alone program linked against the host-only
    sanitized library of `build_sanitized` (built first when it is not current).  Cached by the hash of the library's
    sources and the driver's.  Returns SAN_NAVSIM_DRIVER."""
    import hashlib
    build_sanitized(force=force, verbose=verbose)
    h = hashlib.sha256((source_hash() + open(SAN_NAVSIM_DRIVER_SRC).read()).encode()).hexdigest()
    tag = SAN_NAVSIM_DRIVER + ".srchash"
    try:
        if not force and os.path.exists(SAN_NAVSIM_DRIVER) and open(tag).read().strip() == h:
            return SAN_NAVSIM_DRIVER
    except OSError:
        pass
    clangxx = os.path.join(os.path.dirname(os.path.dirname(hipcc())), "lib", "llvm", "bin", "clang++")
    cmd = [clangxx if os.path.exists(clangxx) else "clang++", "-std=c++17", "-O1", "-g", *SAN_FLAGS, "-o", SAN_NAVSIM_DRIVER,
           SAN_NAVSIM_DRIVER_SRC, SAN_OUT, "-Wl,-rpath," + os.path.dirname(SAN_OUT)]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL if not verbose else None)
    with open(tag, "w") as f:
        f.write(h + "\n")
    return SAN_NAVSIM_DRIVER


# eighth driver, built the same way: the range fill and the keyed sampler of prioritized replay (tests/test_per_vector_host.py)
SAN_PER_VECTOR_DRIVER_SRC = os.path.join(os.path.dirname(HERE), "tests", "helpers", "abi_reject_per_vector.cpp")
SAN_PER_VECTOR_DRIVER = os.path.join(HERE, "lib", "abi_reject_per_vector_san")


def build_sanitized_per_vector(force=False, verbose=True):
    """tests/helpers/abi_reject_per_vector.cpp -> SAN_PER_VECTOR_DRIVER, a stand-alone program linked against the host-only
    sanitized library of `build_sanitized` (built first when it is not current).  Cached by the hash of the library's
    sources and the driver's.  Returns SAN_PER_VECTOR_DRIVER."""
    import hashlib
    build_sanitized(force=force, verbose=verbose)
    h = hashlib.sha256((source_hash() + open(SAN_PER_VECTOR_DRIVER_SRC).read()).encode()).hexdigest()
    tag = SAN_PER_VECTOR_DRIVER + ".srchash"
    try:
        if not force and os.path.exists(SAN_PER_VECTOR_DRIVER) and open(tag).read().strip() == h:
            return SAN_PER_VECTOR_DRIVER
    except OSError:
        pass
    clangxx = os.path.join(os.path.dirname(os.path.dirname(hipcc())), "lib", "llvm", "bin", "clang++")
    cmd = [clangxx if os.path.exists(clangxx) else "clang++", "-std=c++17", "-O1", "-g", *SAN_FLAGS, "-o", SAN_PER_VECTOR_DRIVER,
           SAN_PER_VECTOR_DRIVER_SRC, SAN_OUT, "-Wl,-rpath," + os.path.dirname(SAN_OUT)]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL if not verbose else None)
    with open(tag, "w") as f:
        f.write(h + "\n")
    return SAN_PER_VECTOR_DRIVER


# ninth driver, built the same way: the A* expert's entry points (tests/test_expert_host.py)
SAN_EXPERT_DRIVER_SRC = os.path.join(os.path.dirname(HERE), "tests", "helpers", "abi_reject_expert.cpp")
SAN_EXPERT_DRIVER = os.path.join(HERE, "lib", "abi_reject_expert_san")


def build_sanitized_expert(force=False, verbose=True):
    """tests/helpers/abi_reject_expert.cpp -> SAN_EXPERT_DRIVER, a stand-alone program linked against the host-only
    sanitized library of `build_sanitized` (built first when it is not current).  Cached by the hash of the library's
    sources and the driver's.  Returns SAN_EXPERT_DRIVER."""
    import hashlib
    build_sanitized(force=force, verbose=verbose)
    h = hashlib.sha256((source_hash() + open(SAN_EXPERT_DRIVER_SRC).read()).encode()).hexdigest()
    tag = SAN_EXPERT_DRIVER + ".srchash"
    try:
        if not force and os.path.exists(SAN_EXPERT_DRIVER) and open(tag).read().strip() == h:
            return SAN_EXPERT_DRIVER
    except OSError:
        pass
    clangxx = os.path.join(os.path.dirname(os.path.dirname(hipcc())), "lib", "llvm", "bin", "clang++")
    cmd = [clangxx if os.path.exists(clangxx) else "clang++", "-std=c++17", "-O1", "-g", *SAN_FLAGS, "-o", SAN_EXPERT_DRIVER,
           SAN_EXPERT_DRIVER_SRC, SAN_OUT, "-Wl,-rpath," + os.path.dirname(SAN_OUT)]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL if not verbose else None)
    with open(tag, "w") as f:
        f.write(h + "\n")
    return SAN_EXPERT_DRIVER


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(OUT)
    if "--sanitized" in sys.argv:
        print(build_sanitized(force="--force" in sys.argv))
        print(SAN_ROWS_DRIVER)
        print(SAN_EPISODES_DRIVER)
        print(build_sanitized_holdout(force="--force" in sys.argv))
        print(build_sanitized_normalize(force="--force" in sys.argv))
        print(build_sanitized_goal_bc(force="--force" in sys.argv))
        print(build_sanitized_navsim(force="--force" in sys.argv))
        print(build_sanitized_per_vector(force="--force" in sys.argv))
        print(build_sanitized_expert(force="--force" in sys.argv))
