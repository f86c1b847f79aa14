"""Device cost of the seeded signature clusters (fdgpu_signature_clusters_seeded): a drop made non-redundant against representatives that
already stand.  The signatures are those of --structures synthetic structures (as tools/neighbors_probe.py makes them).  Seeds = the
representatives of the first --seed-from of them at --min-similarity; drops = the first n of the signatures behind those, per --sizes entry.
Per size, in a process of its own (HIP events of fdgpu_last_timings; one warm-up, medians of --runs):
  seeded     the stages of the seeded call: sigcl_seed (+ sigcl_seed_merge), and the walk's sigcl_scan + sigcl_resolve summed over their launches
  (a)        fdgpu_signature_neighbors with k = 1 of the drop against the same seeds: signb_scan (+ signb_merge), the same compares with the
             k-list kernel
  (b)        fdgpu_signature_clusters of [seeds; drop] in that order: what has to be run without a seed table (scan + resolve, and the call)
and whether the device and the host form of the seeded call agree byte for byte.

Every step that uses the GPU is a child process of its own under its own time limit; the first one that fails ends the probe.  One JSON line.

    python tools/cluster_seeded_probe.py [--structures 67750] [--seed-from 60000] [--sizes 1024 4096 7750] [--min-similarity 0.9]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.cluster_probe import timings          # noqa: E402  (every stage of a call summed over its launches)
from tools.neighbors_probe import step_base      # noqa: E402  (the signatures of the synthetic index -> a.base)


def step_seeds(a):
    """the representatives of the first a.seed_from signatures -> a.seeds (.npy)"""
    import folddisco_amd as fd
    from folddisco_amd import indexio
    ctx = fd.Context(0)
    head = np.load(a.base)[:a.seed_from]
    cl = ctx.signature_clusters(head, thr64=indexio.signature_threshold(a.min_similarity))
    reps = head[cl["id"] == np.arange(len(head))]
    np.save(a.seeds, reps)
    return dict(walked=len(head), seeds=len(reps))


def _median_stages(ctx, call, runs, cap):
    call()                                            # the warm-up of the workspaces
    ctx.enable_timing(True)
    got = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        st, launches = timings(ctx, cap)
        st["call_wall"] = (time.perf_counter() - t0) * 1e3
        got.append((st, launches))
    ctx.enable_timing(False)
    return {k: round(float(np.median([g[0].get(k, 0.0) for g in got])), 3) for k in got[0][0]}, got[0][1]


def step_size(a):
    import folddisco_amd as fd
    from folddisco_amd import indexio
    ctx = fd.Context(0)
    seeds = np.load(a.seeds)
    drop = np.ascontiguousarray(np.load(a.base)[a.seed_from:a.seed_from + a.n])
    thr64 = indexio.signature_threshold(a.min_similarity)
    joined = np.concatenate([seeds, drop])
    cap = 16 + 2 * ((len(joined) + 255) // 256)
    got = np.array(ctx.signature_clusters(drop, thr64=thr64, seeds=seeds))
    seeded, launches = _median_stages(ctx, lambda: ctx.signature_clusters(drop, thr64=thr64, seeds=seeds), a.runs, cap)
    near, _ = _median_stages(ctx, lambda: ctx.signature_neighbors(drop, seeds, k=1, thr64=thr64), a.runs, cap)
    whole, whole_launches = _median_stages(ctx, lambda: ctx.signature_clusters(joined, thr64=thr64), a.runs, cap)
    seed_ms = seeded["sigcl_seed"] + seeded.get("sigcl_seed_merge", 0.0)
    walk_ms = seeded.get("sigcl_scan", 0.0) + seeded["sigcl_resolve"]
    near_ms = near["signb_scan"] + near.get("signb_merge", 0.0)
    whole_ms = whole.get("sigcl_scan", 0.0) + whole["sigcl_resolve"]
    t0 = time.perf_counter()
    want = indexio.signature_clusters_host(drop, thr64=thr64, threads=a.host_threads, seeds=seeds)
    host_s = time.perf_counter() - t0
    of_seed = (got["flags"] & indexio.SIG_SEED) != 0
    rep = ~of_seed & (got["id"] == np.arange(len(drop)))
    # the whole walk says the same about the drop: the seeds are mutually non-redundant and walked first, so all of them stand
    tail = np.array(ctx.signature_clusters(joined, thr64=thr64))[len(seeds):]
    same = bool(np.array_equal(tail["id"] < len(seeds), of_seed) and np.array_equal(tail["id"][of_seed], got["id"][of_seed])
                and np.array_equal(tail["id"][~of_seed & (got["id"] != indexio.SIG_NO_ID)] - len(seeds), got["id"][~of_seed & (got["id"] != indexio.SIG_NO_ID)]))
    return dict(seeds=len(seeds), drop=len(drop), members_of_seeds=int(of_seed.sum()), new_representatives=int(rep.sum()),
                seeded=dict(stage_ms=seeded, launches=launches, seed_pass_ms=round(seed_ms, 3), walk_ms=round(walk_ms, 3), device_ms=round(seed_ms + walk_ms, 3)),
                neighbors_k1=dict(stage_ms=near, scan_plus_merge_ms=round(near_ms, 3)), seed_pass_over_neighbors=round(seed_ms / max(near_ms, 1e-6), 3),
                unseeded_whole=dict(stage_ms=whole, launches=whole_launches, scan_plus_resolve_ms=round(whole_ms, 3)),
                whole_over_seeded_device=round(whole_ms / max(seed_ms + walk_ms, 1e-6), 2),
                whole_over_seeded_call=round(whole["call_wall"] / max(seeded["call_wall"], 1e-6), 2),
                host_form_s=round(host_s, 3), host_equals_device=got.tobytes() == want.tobytes(), whole_walk_agrees=same,
                ok=bool(got.tobytes() == want.tobytes() and same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=67750)
    ap.add_argument("--seed-from", type=int, default=60000, help="the seeds are the representatives of this many first signatures")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 7750])
    ap.add_argument("--min-similarity", type=float, default=0.9)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step's child process may take")
    ap.add_argument("--step", choices=["base", "seeds", "size"], default=None, help=argparse.SUPPRESS)      # the child's side
    ap.add_argument("--base", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--seeds", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps({"base": step_base, "seeds": step_seeds, "size": step_size}[a.step](a)), flush=True)
        return 0
    out, ok = dict(structures=a.structures, seed_from=a.seed_from, runs=a.runs, host_threads=a.host_threads, min_similarity=a.min_similarity), True
    with tempfile.TemporaryDirectory() as tmp:
        base, seeds = os.path.join(tmp, "base.npy"), os.path.join(tmp, "seeds.npy")
        common = [sys.executable, os.path.abspath(__file__), "--base", base, "--seeds", seeds, "--structures", str(a.structures), "--seed-from", str(a.seed_from),
                  "--seed", str(a.seed), "--runs", str(a.runs), "--host-threads", str(a.host_threads), "--min-similarity", str(a.min_similarity)]
        steps = [("base", ["--step", "base"]), ("seeds", ["--step", "seeds"])] + [(f"drop_{n}", ["--step", "size", "--n", str(n)]) for n in a.sizes]
        for name, args in steps:
            try:
                r = subprocess.run(common + args, stdout=subprocess.PIPE, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                out[name] = f"no result within {a.step_timeout} s"
                ok = False
                break                              # nothing more is started on the device after a step that hung or failed
            if r.returncode != 0:
                out[name] = f"exit status {r.returncode}"
                ok = False
                break
            out[name] = json.loads(r.stdout.decode().strip().splitlines()[-1])
            ok &= out[name].get("ok", True)
            print(f"[probe] {name}: {json.dumps(out[name])}", file=sys.stderr, flush=True)
    out["host_equals_device"] = "pass" if ok else "FAIL"
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
