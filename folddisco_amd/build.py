"""Builds folddisco_amd/libfdgpu.so (gfx950) in-tree with hipcc.

Flags that matter for bit-parity with the reference (see csrc/fd_libm.h):
  -ffp-contract=off   no FMA contraction: every f32/f64 op rounds like the Rust/glibc original
  (no -ffast-math)    IEEE division and sqrt (hipcc default: correctly rounded), denormals kept
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libfdgpu.so")
# k_hash.hip: the SLP vectoriser packs the pair geometry into v_pk_* ops at the price of ~2 v_mov per packed op; the pair
# kernel is VALU-issue bound, scalar code is ~10 % fewer instructions (measured faster)
EXTRA_FLAGS = {"k_hash.hip": os.environ.get("FD_KHASH_FLAGS", "-fno-slp-vectorize").split()}
SOURCES = ["fdgpu_api.hip", "fd_api_build.hip", "fd_api_count.hip", "fd_api_match.hip", "k_hash.hip", "k_sort.hip", "k_index.hip", "k_merge.hip", "k_query.hip", "k_qtile.hip", "k_qscore32.hip", "k_match.hip", "k_retrieve.hip", "fd_query_map.hip", "fd_host_query.hip", "fd_comm.hip", "fd_lanes.hip", "fd_shard_index.hip", "k_prune.hip", "k_split.hip", "k_rebase.hip", "k_permute.hip", "k_rows.hip", "k_sig.hip", "k_overlap.hip", "k_exact.hip", "k_verify.hip", "k_batch.hip", "fd_verify_host.cpp", "fd_split_host.cpp", "fd_rebase_host.cpp", "fd_permute_host.cpp", "fd_rows_host.cpp", "fd_signatures_host.cpp", "fd_overlap_host.cpp", "fd_neighbors_exact_host.cpp", "fd_retrieve_host.cpp", "fd_match_tables.cpp", "fd_query_map_host.cpp", "fd_ingest.cpp", "fd_inflate.cpp", "fd_fcz.cpp"]


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "fdgpu.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    srcs = [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for s in srcs:
        o = os.path.join(HERE, "build", os.path.basename(s) + ".o")
        cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
               "-fgpu-rdc" if False else "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"] + EXTRA_FLAGS.get(os.path.basename(s), []) + ["-c", s, "-o", o]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((subprocess.Popen(cmd), s))
        objs.append(o)
    for p, s in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {s}")
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-lz", "-lpthread", "-ldl"]
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
