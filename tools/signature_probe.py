"""Device cost of index signatures and of their compare: build --structures synthetic structures resident, take the signatures
(fdgpu_index_signatures) of a window of each --window width from the middle of the index and the rows (fdgpu_index_rows) of the same window,
--runs times each, then compare signature tables of each --pairs size in self mode (fdgpu_signature_pairs) against the host form.  Prints one
JSON line with the per-stage device times (HIP events of fdgpu_last_timings, not host clocks around asynchronous calls; medians over the
runs) of both calls over the same window (the stages up to rows_bounds are the same code; the signatures end in sig_reduce + sig_copy, the rows
in rows_copy), the compare's stages and pair rate per table size, the wall time of the host forms, and a check that device and host agree.

    python tools/signature_probe.py [--structures 67750] [--window 16384] [--pairs 4096 16384 65536] [--host-pairs-max 16384] [--runs 3] [--host-threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEN_BLOCK = 67750          # structures per generated block = per build call (bench.py's block)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=67750)
    ap.add_argument("--window", type=int, nargs="+", default=[16384], help="window widths to measure, each taken from the middle of the index")
    ap.add_argument("--pairs", type=int, nargs="+", default=[4096, 16384, 65536], help="table sizes of the self compare (the index's signatures, repeated with "
                    "their sketches redrawn beyond --structures)")
    ap.add_argument("--host-pairs-max", type=int, default=16384, help="largest table the host compare is timed on (it is quadratic)")
    ap.add_argument("--min-similarity", type=float, default=0.9)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    import folddisco_amd as fd
    from folddisco_amd import indexio, synth
    dev = torch.device("cuda", 0)
    ctx = fd.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)

    def wrap(d):
        ro = d["res_off"].contiguous()
        n = len(ro) - 1
        return ctx.wrap_device(n, int(ro[-1].item()), ro.data_ptr(), d["n_xyz"].data_ptr(), d["ca_xyz"].data_ptr(), d["cb_xyz"].data_ptr(),
                               d["aa"].data_ptr(), None, keepalive=(ro, d))

    def timed():
        ctx.synchronize()
        t = {}
        for n, ms, _ in ctx.last_timings():       # the sort's stages recur once per pass: summed per name
            t[n] = t.get(n, 0.0) + ms
        return t

    def measure(f):
        f()                                       # the warm-up of the workspaces
        ctx.enable_timing(True)
        runs, wall = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            r = f()
            wall.append(time.perf_counter() - t0)
            runs.append(timed())
            del r
        ctx.enable_timing(False)
        med = lambda xs: float(np.median(xs))
        return dict(stage_ms={k: round(med([r[k] for r in runs]), 3) for k in runs[0]}, device_ms=round(med([sum(r.values()) for r in runs]), 3),
                    wall_ms=round(med(wall) * 1e3, 3))

    parts, fid = [], 0
    for b in range(0, a.structures, GEN_BLOCK):
        n = min(GEN_BLOCK, a.structures - b)
        d = synth.generate(n, seed=a.seed + 1000 * (b // GEN_BLOCK), device=dev)
        parts.append(fd.FolddiscoIndex.build(ctx, wrap(d), first_id=fid))
        fid += n
        del d
    ix = fd.FolddiscoIndexSet(parts).merge() if len(parts) > 1 else parts[0]
    del parts
    ctx.synchronize()
    ctx.release_workspaces()
    S = a.structures
    out = dict(structures=S, runs=a.runs, V=ix.value_len, hashes=ix.num_hashes, postings=ix.num_postings, host_threads=a.host_threads)
    ok = True
    src = ix.export_view()
    for w in a.window:
        w = min(w, S)
        w0 = (S - w) // 2
        got = np.array(ix.signatures(w0, w0 + w, window=w))
        t0 = time.perf_counter()
        want = indexio.signatures_host(*src, S, lo=w0, hi=w0 + w, threads=a.host_threads)
        host_s = time.perf_counter() - t0
        ok &= got.tobytes() == want.tobytes()
        out[f"window_{w}"] = dict(lo=w0, hi=w0 + w, postings=int(got["n"].sum()), longest_row=int(got["n"].max()),
                                  signatures=measure(lambda: ix.signatures(w0, w0 + w, window=w)), rows=measure(lambda: ix.rows(w0, w0 + w)),
                                  host_form_s=round(host_s, 3))
        del got, want
    del src
    base = np.array(ix.signatures())
    del ix
    ctx.release_workspaces()
    thr64 = indexio.signature_threshold(a.min_similarity)
    rng = np.random.Generator(np.random.PCG64(a.seed))
    for n in a.pairs:
        T = np.resize(base, n)
        if n > S:                                 # the repeats get sketches of their own: a table of copies would report every copy pair
            T["sk"][S:] = rng.integers(0, 0xffffffff, size=(n - S, 64), dtype=np.uint64).astype(np.uint32)
        got = ctx.signature_pairs(T, thr64=thr64)
        rec = dict(pairs_compared=n * (n - 1) // 2, reported=len(got), thr64=thr64, **measure(lambda: ctx.signature_pairs(T, thr64=thr64)))
        rec["Gpairs_per_s"] = round(rec["pairs_compared"] / (rec["stage_ms"]["sigpairs_match"] * 1e-3) / 1e9, 2)
        if n <= a.host_pairs_max:
            t0 = time.perf_counter()
            want = indexio.signature_pairs_host(T, thr64=thr64, threads=a.host_threads)
            rec["host_form_s"] = round(time.perf_counter() - t0, 3)
            ok &= got.tobytes() == want.tobytes()
        out[f"pairs_{n}"] = rec
    out["host_equals_device"] = "pass" if ok else "FAIL"
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
