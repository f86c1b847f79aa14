"""Device cost of index rows at database scale: build --structures synthetic structures resident, take the rows (fdgpu_index_rows) of a window
of each --window width from the middle of the index and, with --whole, of the whole index, --runs times each.  Prints one JSON line with the
per-stage device times (HIP events of fdgpu_last_timings, not host clocks around asynchronous calls; medians over the runs), the bytes the
plan states for each (value bytes read twice, 8 bytes per window posting emitted, 16 bytes per window posting and sort pass), the wall time of
the host form (fdgpu_rows_host, --host-threads threads) for the same window, and a check that both forms give the same arrays.

    python tools/rows_probe.py [--structures 203250] [--window 16384 65536] [--whole] [--runs 3] [--host-threads 16] [--seed 7]
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
    ap.add_argument("--structures", type=int, default=203250)
    ap.add_argument("--window", type=int, nargs="+", default=[16384], help="window widths to measure, each taken from the middle of the index")
    ap.add_argument("--whole", action="store_true", help="also take the rows of the whole index")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-whole", action="store_true", help="time the host form on the whole index as well (minutes at database scale)")
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
        for n, ms, b in ctx.last_timings():       # the sort's stages recur once per pass: summed per name
            t[n] = (t.get(n, (0.0, 0))[0] + ms, t.get(n, (0.0, 0))[1] + b)
        return t

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
    S, V, H = a.structures, ix.value_len, ix.num_hashes
    windows = [(f"window_{min(w, S)}", (S - min(w, S)) // 2, (S - min(w, S)) // 2 + min(w, S)) for w in a.window] + ([("whole", 0, S)] if a.whole else [])
    src = ix.export_view()
    med = lambda xs: float(np.median(xs))
    out = dict(structures=S, runs=a.runs, V=V, hashes=H, postings=ix.num_postings, host_threads=a.host_threads)
    ok = True
    for name, w0, w1 in windows:
        try:
            got = ix.rows(w0, w1)                 # the warm-up of the workspaces, and the arrays of the check
        except fd.FdgpuError as e:                # 2^32 postings in one window: the documented refusal, not a failure of the probe
            out[name] = dict(lo=w0, hi=w1, refused=str(e))
            continue
        n = len(got[0])
        host_s = None
        if name != "whole" or a.host_whole:
            t0 = time.perf_counter()
            want = indexio.rows_host(*src, S, lo=w0, hi=w1, threads=a.host_threads)
            host_s = time.perf_counter() - t0
            ok &= np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            del want
        del got
        ctx.enable_timing(True)
        runs, wall = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            r = ix.rows(w0, w1)
            wall.append(time.perf_counter() - t0)
            runs.append(timed())
            del r
        ctx.enable_timing(False)
        stage = {k: round(med([r[k][0] for r in runs]), 3) for k in runs[0]}
        device_ms = med([sum(ms for ms, _ in r.values()) for r in runs])
        passes = 0
        while (1 << (8 * passes)) < (w1 - w0):
            passes += 1
        model = 2 * V + 8 * n + 16 * n * passes
        out[name] = dict(lo=w0, hi=w1, postings=n, sort_passes=passes, stage_ms=stage, device_ms=round(device_ms, 3), wall_ms=round(med(wall) * 1e3, 3),
                         model_bytes=model, model_GBps=round(model / (device_ms * 1e-3) / 1e9, 1),
                         host_form_s=None if host_s is None else round(host_s, 3))
    out["host_equals_device"] = "pass" if ok else "FAIL"
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
