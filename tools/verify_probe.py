"""Device cost of fdgpu_index_verify at database scale, beside the two full passes over the same bytes that exist already.

Builds --structures synthetic structures resident (blocks merged on the device, like tools/update_probe.py), warms the check up once and
repeats it --reps times: per-stage device times (HIP events of fdgpu_last_timings) as min / median / max, and the rate over
value_len + 12 H bytes (the value bytes, 8 bytes of offsets and 4 of hashes per list).  Then the index is exported, loaded again
(fdgpu_index_load: the terminator count k_count_postings, one streaming read of the value bytes — the floor) and one structure is removed
from the loaded copy (the first removal derives the per-list last ids: k_mg_last_ids, a wavefront per list over the same bytes), and the
loaded copy is verified too.  Host clocks around those two calls are printed for orientation only (they include the copies); the kernels'
own times come from a trace run of this program, where k_vf_table / k_vf_lists appear beside them:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o verify -- python tools/verify_probe.py [--structures 542000]
    python tools/verify_probe.py --stats OUT      # condenses the trace: the four kernels, calls, average and total time

Prints one JSON line.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEN_BLOCK = 67750          # structures per generated block = per build call (bench.py's block)
HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes/s (spec)
KERNELS = ("k_vf_table", "k_vf_lists", "k_count_postings", "k_mg_last_ids")


def condense(raw):
    out = {}
    for f in sorted(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            nm = r.get("Name", "").replace("void ", "").split("(")[0]
            if nm in KERNELS:
                out[nm] = dict(calls=int(r["Calls"]), avg_ms=round(float(r["AverageNs"]) / 1e6, 3), min_ms=round(float(r["MinNs"]) / 1e6, 3),
                               max_ms=round(float(r["MaxNs"]) / 1e6, 3), total_ms=round(float(r["TotalDurationNs"]) / 1e6, 3))
    print(json.dumps(dict(kernel_trace=out)), flush=True)
    return 0 if len(out) == len(KERNELS) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=542000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--stats", default="", help="condense the kernel trace under this directory instead of running")
    a = ap.parse_args()
    if a.stats:
        return condense(a.stats)
    import torch
    import folddisco_amd as fd
    from folddisco_amd import synth
    dev = torch.device("cuda", 0)
    ctx = fd.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)

    def wrap(d):
        ro = d["res_off"].contiguous()
        n = len(ro) - 1
        return ctx.wrap_device(n, int(ro[-1].item()), ro.data_ptr(), d["n_xyz"].data_ptr(), d["ca_xyz"].data_ptr(), d["cb_xyz"].data_ptr(),
                               d["aa"].data_ptr(), None, keepalive=(ro, d))

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
    V, H = ix.value_len, ix.num_hashes

    def verify_timed(index, reps):
        ctx.enable_timing(True)
        rep = index.verify()                 # warm-up: code objects, workspaces
        stages = {}
        for _ in range(reps):
            rep = index.verify()
            ctx.synchronize()
            for name, ms, _ in ctx.last_timings():
                stages.setdefault(name, []).append(ms)
        ctx.enable_timing(False)
        return rep, {k: dict(min=round(min(v), 3), median=round(statistics.median(v), 3), max=round(max(v), 3)) for k, v in stages.items()}

    rep, st = verify_timed(ix, a.reps)
    total = sum(s["median"] for s in st.values())
    out = dict(structures=a.structures, hashes=H, value_bytes=V, reps=a.reps, verdict=str(rep), ok=rep.ok, postings_match=rep.n_postings == ix.num_postings,
               longest_list_bytes=rep.max_list_bytes, verify_stages_ms=st, verify_ms=round(total, 3),
               verify_GBps=round((V + 12 * H) / (total * 1e-3) / 1e9, 1), verify_hbm_peak_fraction=round((V + 12 * H) / (total * 1e-3) / HBM_PEAK, 4))
    # the two existing full passes over the same bytes, through calls that exist
    v, h, o = ix.export_view()          # no second host copy of the value bytes
    del ix
    ctx.release_workspaces()
    t0 = time.perf_counter()
    loaded = fd.FolddiscoIndex.load(ctx, h, o, v, a.structures)          # k_count_postings
    ctx.synchronize()
    out["load_host_s"] = round(time.perf_counter() - t0, 3)
    del v, h, o
    rep2, st2 = verify_timed(loaded, min(a.reps, 3))
    out["loaded_verify_stages_ms"] = st2
    out["loaded_ok"] = rep2.ok and rep2.n_postings == loaded.num_postings
    keep = np.ones(a.structures, bool)
    keep[a.structures // 2] = False
    t0 = time.perf_counter()
    pruned = loaded.remove(keep)                                         # k_mg_last_ids, then the prune
    ctx.synchronize()
    out["remove_one_host_s"] = round(time.perf_counter() - t0, 3)
    out["pruned_ok"] = pruned.verify().ok
    print(json.dumps(out), flush=True)
    return 0 if out["ok"] and out["postings_match"] and out["loaded_ok"] and out["pruned_ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
