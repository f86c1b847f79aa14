"""Device cost of the signature neighbours (fdgpu_signature_neighbors) beside the bare compare loop of fdgpu_signature_pairs.  The tables are
those of tools/signature_probe.py: the signatures of --structures synthetic structures, repeated with their sketches redrawn beyond that
number (the redrawn records agree with nobody: they are candidates of no query, so beyond --structures the selection has nothing to insert).
Per --sizes entry and per --k: the neighbours inside the table (both triangles: n (n - 1) candidate pairs), their stages as device times (HIP
events of fdgpu_last_timings; one warm-up, medians of --runs), candidate pairs per second, and as yardstick sigpairs_match of the self compare
at thr64 = 64 over the same table (n (n - 1) / 2 pairs, next to nothing reported); `ratio` is the cost per pair visited, neighbours over
yardstick.  Then --queries signatures against the largest table (two-table mode: the split and the merge), and the host form at the sizes up
to --host-max with a check that device and host agree byte for byte.

Every step that uses the GPU is a child process of its own under its own time limit; the first one that fails ends the probe.  One JSON line.

    python tools/neighbors_probe.py [--structures 67750] [--sizes 4096 16384 65536 262144 542000] [--k 8 32] [--queries 1024] [--host-max 16384]
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

GEN_BLOCK = 67750          # structures per generated block = per build call (bench.py's block)


def table(base, n, seed):
    T = np.resize(base, n)
    S = len(base)
    if n > S:
        rng = np.random.Generator(np.random.PCG64(seed))
        T["sk"][S:] = rng.integers(0, 0xffffffff, size=(n - S, 64), dtype=np.uint64).astype(np.uint32)
    return T


def step_base(a):
    """the signatures of the synthetic index -> a.base (.npy)"""
    import torch
    import folddisco_amd as fd
    from folddisco_amd import synth
    dev = torch.device("cuda", 0)
    ctx = fd.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    parts, fid = [], 0
    for b in range(0, a.structures, GEN_BLOCK):
        n = min(GEN_BLOCK, a.structures - b)
        d = synth.generate(n, seed=a.seed + 1000 * (b // GEN_BLOCK), device=dev)
        ro = d["res_off"].contiguous()
        batch = ctx.wrap_device(len(ro) - 1, int(ro[-1].item()), ro.data_ptr(), d["n_xyz"].data_ptr(), d["ca_xyz"].data_ptr(), d["cb_xyz"].data_ptr(),
                                d["aa"].data_ptr(), None, keepalive=(ro, d))
        parts.append(fd.FolddiscoIndex.build(ctx, batch, first_id=fid))
        fid += n
    ix = fd.FolddiscoIndexSet(parts).merge() if len(parts) > 1 else parts[0]
    np.save(a.base, np.array(ix.signatures()))
    return dict(structures=a.structures)


def step_size(a):
    """one table size (a.n), or a.queries signatures of it against the whole of it when a.two"""
    import folddisco_amd as fd
    from folddisco_amd import indexio
    ctx = fd.Context(0)
    T = table(np.load(a.base), a.n, a.seed)

    def measure(f):
        f()                                       # the warm-up of the workspaces
        ctx.enable_timing(True)
        runs = []
        for _ in range(a.runs):
            f()
            ctx.synchronize()
            runs.append({n: ms for n, ms, _ in ctx.last_timings()})
        ctx.enable_timing(False)
        return {k: round(float(np.median([r[k] for r in runs])), 3) for k in runs[0]}

    out, ok = {}, True
    if a.two:
        real = min(a.n, a.structures)                   # queries from the index's own signatures: they have neighbours
        Q = T[:real][:: max(real // a.queries, 1)][:a.queries].copy()
        visited = len(Q) * a.n
    else:
        Q, visited = T, a.n * (a.n - 1)
        y = measure(lambda: ctx.signature_pairs(T, thr64=64))
        out["yardstick"] = dict(pairs=visited // 2, sigpairs_match_ms=y["sigpairs_match"], ns_per_pair=round(y["sigpairs_match"] * 1e6 / max(visited // 2, 1), 5))
    for k in a.k:
        f = (lambda: ctx.signature_neighbors(Q, T, k=k)) if a.two else (lambda: ctx.signature_neighbors(T, k=k))
        got = np.array(f())
        st = measure(f)
        rec = dict(pairs=visited, stage_ms=st, Gpairs_per_s=round(visited / (st["signb_scan"] * 1e-3) / 1e9, 2), ns_per_pair=round(st["signb_scan"] * 1e6 / max(visited, 1), 5),
                   with_k_neighbours=int((got["id"][:, -1] != indexio.SIG_NO_ID).sum()), without_any=int((got["id"][:, 0] == indexio.SIG_NO_ID).sum()))
        if not a.two:
            rec["ratio"] = round(rec["ns_per_pair"] / out["yardstick"]["ns_per_pair"], 3)
        if a.two or a.n <= a.host_max:
            t0 = time.perf_counter()
            want = indexio.signature_neighbors_host(Q, T if a.two else None, k=k, threads=a.host_threads)
            rec["host_form_s"] = round(time.perf_counter() - t0, 3)
            ok &= got.tobytes() == want.tobytes()
            rec["host_equals_device"] = got.tobytes() == want.tobytes()
        out[f"k_{k}"] = rec
    out["ok"] = bool(ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=67750)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384, 65536, 262144, 542000])
    ap.add_argument("--k", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--queries", type=int, default=1024, help="query table of the two-table step, against the largest of --sizes")
    ap.add_argument("--host-max", type=int, default=16384, help="largest table the host form is timed on (it is quadratic)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step's child process may take")
    ap.add_argument("--step", choices=["base", "size"], default=None, help=argparse.SUPPRESS)      # the child's side
    ap.add_argument("--base", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--two", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps((step_base if a.step == "base" else step_size)(a)), flush=True)
        return 0
    out, ok = dict(structures=a.structures, runs=a.runs, host_threads=a.host_threads), True
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base.npy")
        common = [sys.executable, os.path.abspath(__file__), "--base", base, "--structures", str(a.structures), "--seed", str(a.seed), "--runs", str(a.runs),
                  "--host-threads", str(a.host_threads), "--host-max", str(a.host_max), "--queries", str(a.queries), "--k", *map(str, a.k)]
        steps = [("base", ["--step", "base"])] + [(f"self_{n}", ["--step", "size", "--n", str(n)]) for n in a.sizes]
        steps.append((f"two_{a.queries}x{max(a.sizes)}", ["--step", "size", "--n", str(max(a.sizes)), "--two"]))
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
