"""Device cost of the signature clusters (fdgpu_signature_clusters) beside the all-against-all compare of fdgpu_signature_pairs over the same
table.  The table holds the signatures of --structures synthetic structures (as tools/neighbors_probe.py makes them), the first n / copies of
them `copies` times each in a seeded random order: copies = 1 makes nearly every structure a representative (the clustering then visits
every pair once, as the compare does), copies = 4 a quarter of them (it visits a quarter of the pairs).  Per --sizes entry and per --copies:
the stages of the device form summed over their launches (HIP events of fdgpu_last_timings; one warm-up, medians of --runs), the number of
launches and of representatives, `sigpairs_match` of the self compare at the same threshold over the same table (the yardstick; its pairs are
counted, at most --max-pairs of them kept), and the host form's wall time with a check that device and host agree byte for byte (sizes up to
--host-max).

Every step that uses the GPU is a child process of its own under its own time limit; the first one that fails ends the probe.  One JSON line.

    python tools/cluster_probe.py [--structures 67750] [--sizes 4096 16384 65536] [--copies 1 4] [--min-similarity 0.9] [--host-max 65536]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.neighbors_probe import step_base      # noqa: E402  (the signatures of the synthetic index -> a.base)


def table(base, n, copies, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    T = np.resize(base[:max(n // copies, 1)], n)
    return T[rng.permutation(n)]


def timings(ctx, cap):
    """every stage of the last call, not only the first 64: the clustering records two per block of 256 positions"""
    names, ms = (C.c_char_p * cap)(), (C.c_float * cap)()
    k = ctx.L.fdgpu_last_timings(ctx.h, names, ms, None, cap)
    out, launches = {}, 0
    for i in range(k):
        s = names[i].decode()
        out[s] = out.get(s, 0.0) + float(ms[i])
        launches += s in ("sigcl_scan", "sigcl_resolve")
    return out, launches


def step_size(a):
    import folddisco_amd as fd
    from folddisco_amd import indexio
    ctx = fd.Context(0)
    base = np.load(a.base)
    thr64 = indexio.signature_threshold(a.min_similarity)
    out, ok = {}, True
    for copies in a.copies:
        T = table(base, a.n, copies, a.seed)
        cap = 8 + 2 * ((a.n + 255) // 256)
        got = np.array(ctx.signature_clusters(T, thr64=thr64))      # the warm-up of the workspaces
        ctx.enable_timing(True)
        runs = []
        for _ in range(a.runs):
            ctx.signature_clusters(T, thr64=thr64)
            ctx.synchronize()
            runs.append(timings(ctx, cap))
        stage = {k: round(float(np.median([r[0][k] for r in runs])), 3) for k in runs[0][0]}
        yard = []
        try:
            ctx.signature_pairs(T, thr64=thr64, max_pairs=a.max_pairs)
            for _ in range(a.runs):
                ctx.signature_pairs(T, thr64=thr64, max_pairs=a.max_pairs)
                yard.append(dict((s, ms) for s, ms, _ in ctx.last_timings())["sigpairs_match"])
            pairs = "kept"
        except indexio.SignaturePairsOverflow as e:                  # the kernel ran and counted; nothing beyond max_pairs was written
            for _ in range(a.runs):
                try:
                    ctx.signature_pairs(T, thr64=thr64, max_pairs=a.max_pairs)
                except indexio.SignaturePairsOverflow:
                    pass
                yard.append(dict((s, ms) for s, ms, _ in ctx.last_timings())["sigpairs_match"])
            pairs = f"{e.count} counted"
        ctx.enable_timing(False)
        ids = np.arange(a.n)
        n_rep = int((got["id"] == ids).sum())
        device_ms = stage.get("sigcl_scan", 0.0) + stage["sigcl_resolve"]
        rec = dict(representatives=n_rep, launches=runs[0][1], stage_ms=stage, scan_plus_resolve_ms=round(device_ms, 3),
                   sigpairs_match_ms=round(float(np.median(yard)), 3), sigpairs=pairs,
                   clusters_over_compare=round(device_ms / max(float(np.median(yard)), 1e-6), 3))
        if a.n <= a.host_max:
            t0 = time.perf_counter()
            want = indexio.signature_clusters_host(T, thr64=thr64, threads=a.host_threads)
            rec["host_form_s"] = round(time.perf_counter() - t0, 3)
            rec["host_equals_device"] = got.tobytes() == want.tobytes()
            ok &= rec["host_equals_device"]
        out[f"copies_{copies}"] = rec
    out["ok"] = bool(ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=67750)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--copies", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--min-similarity", type=float, default=0.9)
    ap.add_argument("--max-pairs", type=int, default=1 << 24)
    ap.add_argument("--host-max", type=int, default=65536, help="largest table the host form is timed on")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step's child process may take")
    ap.add_argument("--step", choices=["base", "size"], default=None, help=argparse.SUPPRESS)      # the child's side
    ap.add_argument("--base", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps((step_base if a.step == "base" else step_size)(a)), flush=True)
        return 0
    out, ok = dict(structures=a.structures, runs=a.runs, host_threads=a.host_threads, min_similarity=a.min_similarity), True
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base.npy")
        common = [sys.executable, os.path.abspath(__file__), "--base", base, "--structures", str(a.structures), "--seed", str(a.seed), "--runs", str(a.runs),
                  "--host-threads", str(a.host_threads), "--host-max", str(a.host_max), "--min-similarity", str(a.min_similarity), "--max-pairs", str(a.max_pairs),
                  "--copies", *map(str, a.copies)]
        steps = [("base", ["--step", "base"])] + [(f"n_{n}", ["--step", "size", "--n", str(n)]) for n in a.sizes]
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
