"""Device cost of the exact row overlaps (fdgpu_index_rowset, fdgpu_rowset_intersect) on the synthetic index of --structures structures (as
tools/rows_probe.py builds it).  Per --sizes entry P: a seeded list of P pairs over --rows distinct structures spread over the whole index;
the row set of those structures is built (stages rows_*, rowset_scan, rowset_gather summed over the windows) and the pairs intersected
(overlap_upload, overlap_plan, the sort, overlap_pairs, overlap_copy) — HIP events of fdgpu_last_timings, one warm-up, medians of --runs.
Reported with them: the bytes of the two rows of every pair (4 (|R_a| + |R_b|): what the walk reads at most, it stops where either row ends) and
that figure over the overlap_pairs time, the host form (fdgpu_rows_intersect_host on --host-threads threads over the exported set) with a check
that it equals the device, and, on the smallest size only, the path `--confirm` took before: the windows' rows copied out (fdgpu_index_rows),
the wanted ones kept in a dict, np.intersect1d per pair in a Python loop.

Every size is a child process of its own (it builds the index, measures, and ends) under its own time limit; the first one that fails ends the probe.  One JSON line,
also written to --out if given.

    python tools/overlap_probe.py [--structures 67750] [--rows 4096] [--sizes 1024 16384 262144] [--out profiles/overlap_probe_S67750.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEN_BLOCK = 67750          # structures per generated block = per build call (bench.py's block)


def build_index(a):
    """the synthetic index, resident -> (context, index)"""
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
    del parts
    ctx.synchronize()
    ctx.release_workspaces()
    return ctx, ix


def stages(ctx, cap=1024):
    """every stage of the last call, not only the first 64; the rows' stages recur once per window, the sort's once per pass: summed per name"""
    names, ms = (C.c_char_p * cap)(), (C.c_float * cap)()
    k = ctx.L.fdgpu_last_timings(ctx.h, names, ms, None, cap)
    t = {}
    for i in range(k):
        t[names[i].decode()] = t.get(names[i].decode(), 0.0) + float(ms[i])
    return t


def step_size(a):
    from folddisco_amd import indexio
    ctx, ix = build_index(a)
    rng = np.random.Generator(np.random.PCG64(a.seed))
    ids = np.sort(rng.choice(a.structures, size=min(a.rows, a.structures), replace=False))
    ka, kb = (rng.integers(0, len(ids), size=a.n).astype(np.uint32) for _ in range(2))
    med = lambda xs: float(np.median(xs))
    A, _ = ix.rowset(ids, window=a.window)         # the warm-up of the workspaces
    A.close()
    ctx.enable_timing(True)
    sets = []
    for _ in range(a.runs):
        A, taken = ix.rowset(ids, window=a.window)
        sets.append(stages(ctx))
        if len(sets) < a.runs:
            A.close()
    lens = A.lengths().astype(np.int64)
    ctx.rowset_intersect(A, None, ka, kb)
    runs = []
    for _ in range(a.runs):
        got = np.array(ctx.rowset_intersect(A, None, ka, kb))
        runs.append(stages(ctx))
    ctx.enable_timing(False)
    set_ms = {k: round(med([r[k] for r in sets]), 3) for k in sets[0]}
    ov_ms = {k: round(med([r[k] for r in runs]), 3) for k in runs[0]}
    pair_bytes = int(4 * (lens[ka] + lens[kb]).sum())
    rows = A.export()
    t0 = time.perf_counter()
    want = indexio.rows_intersect_host(rows, None, ka, kb, threads=a.host_threads)
    host_s = time.perf_counter() - t0
    ok = bool(np.array_equal(got, want))
    out = dict(pairs=a.n, V=ix.value_len, hashes=ix.num_hashes, postings=ix.num_postings, distinct_rows=int(taken), set_hashes=int(A.n_hashes), longest_row=int(lens.max()), rowset_stage_ms=set_ms,
               rowset_ms=round(sum(set_ms.values()), 3), overlap_stage_ms=ov_ms, overlap_ms=round(sum(ov_ms.values()), 3),
               pair_row_bytes=pair_bytes, overlap_pairs_GBps=round(pair_bytes / max(ov_ms["overlap_pairs"], 1e-6) / 1e6, 1),
               host_form_s=round(host_s, 3), host_threads=a.host_threads, host_equals_device=ok)
    A.close()
    if a.yardstick:                                # what --confirm did before: rows out of the device into a dict, a Python loop over the pairs
        from folddisco_amd.__main__ import _windows
        t0 = time.perf_counter()
        piece = {}
        for lo, hi, k0, k1 in _windows(ids, a.window, a.structures):
            wh, woff = ix.rows(lo, hi)
            for k in range(k0, k1):
                s = int(ids[k]) - lo
                piece[k] = np.array(wh[int(woff[s]):int(woff[s + 1])])
        t1 = time.perf_counter()
        old = np.array([len(np.intersect1d(piece[int(x)], piece[int(y)])) for x, y in zip(ka, kb)], np.uint32)
        t2 = time.perf_counter()
        ok &= bool(np.array_equal(old, got))
        out["confirm_path_before"] = dict(rows_out_s=round(t1 - t0, 3), intersect1d_loop_s=round(t2 - t1, 3), equals_device=bool(np.array_equal(old, got)))
        out["before_over_now"] = round((t2 - t0) / max((out["rowset_ms"] + out["overlap_ms"]) * 1e-3, 1e-9), 1)
    out["ok"] = ok
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=67750)
    ap.add_argument("--rows", type=int, default=4096, help="distinct structures the pairs are drawn over")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 16384, 262144])
    ap.add_argument("--window", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step's child process may take")
    ap.add_argument("--step", choices=["size"], default=None, help=argparse.SUPPRESS)      # the child's side
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--yardstick", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps(step_size(a)), flush=True)
        return 0
    out, ok = dict(structures=a.structures, rows=a.rows, window=a.window, runs=a.runs, host_threads=a.host_threads), True
    common = [sys.executable, os.path.abspath(__file__), "--structures", str(a.structures), "--rows", str(a.rows), "--seed", str(a.seed),
              "--runs", str(a.runs), "--host-threads", str(a.host_threads), "--window", str(a.window)]
    steps = [(f"pairs_{n}", ["--step", "size", "--n", str(n)] + (["--yardstick"] if n == min(a.sizes) else [])) for n in a.sizes]
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
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
