"""Device cost of an index rebase at database scale: build --structures synthetic structures resident, move the index to another id range
(fdgpu_index_rebase) --runs times, and for comparison run fdgpu_index_merge over that index as a single part in the same process: the same
read-once, write-once byte work in code the library already had.  Prints one JSON line with the per-stage device times (HIP events of
fdgpu_last_timings, not host clocks around asynchronous calls; medians over the runs), each call's rate on the model one read + one write of the
value bytes, and a check that the rebase there and back is the source (byte for byte up to --full-check-bytes; sizes, posting counts and the
verdict of verify beyond).

    python tools/rebase_probe.py [--structures 542000] [--shift 1000000] [--runs 3] [--seed 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEN_BLOCK = 67750          # structures per generated block = per build call (bench.py's block)
HBM_PEAK = 8.0e12          # MI355X HBM3E, bytes/s (spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=542000)
    ap.add_argument("--shift", type=int, default=1000000, help="new first id (the index is built at 0)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--full-check-bytes", type=int, default=4 << 30, help="compare the index moved there and back with the source byte for byte up to this many value bytes")
    a = ap.parse_args()
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

    def timed():
        ctx.synchronize()
        return {n: (ms, b) for n, ms, b in ctx.last_timings()}

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
    ok = True
    got = ix.rebase(a.shift)                      # the check, and the warm-up of the workspaces
    back = got.rebase(0)
    v_new = got.value_len
    ok &= got.num_postings == ix.num_postings == back.num_postings and got.num_hashes == H and back.value_len == V
    if V <= a.full_check_bytes:
        ok &= all(np.array_equal(x, y) for x, y in zip(back.export_view(), ix.export_view()))
    else:
        ok &= got.verify().ok and back.verify().ok
    del got, back
    m = fd.FolddiscoIndexSet([ix]).merge()
    del m
    ctx.enable_timing(True)
    rebase_runs, merge_runs = [], []
    for _ in range(a.runs):
        got = ix.rebase(a.shift)
        rebase_runs.append(timed())
        del got
        m = fd.FolddiscoIndexSet([ix]).merge()
        merge_runs.append(timed())
        del m
    ctx.enable_timing(False)
    med = lambda xs: float(np.median(xs))

    def stages(runs):
        return {n: round(med([r[n][0] for r in runs]), 3) for n in runs[0]}
    rebase_ms = med([sum(ms for ms, _ in r.values()) for r in rebase_runs])
    merge_ms = med([sum(ms for ms, _ in r.values()) for r in merge_runs])
    model = V + v_new
    out = dict(structures=a.structures, shift=a.shift, runs=a.runs, V=V, V_rebased=v_new, hashes=H, rebase_ms=round(rebase_ms, 3), rebase_stage_ms=stages(rebase_runs),
               rebase_model_GBps=round(model / (rebase_ms * 1e-3) / 1e9, 1), rebase_hbm_peak_fraction=round(model / (rebase_ms * 1e-3) / HBM_PEAK, 3),
               merge_single_part_ms=round(merge_ms, 3), merge_stage_ms=stages(merge_runs), merge_model_GBps=round(2 * V / (merge_ms * 1e-3) / 1e9, 1),
               rebase_over_merge=round(rebase_ms / merge_ms, 2), round_trip_check="pass" if ok else "FAIL")
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
