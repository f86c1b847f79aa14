"""Device cost of an index split at database scale: build --structures synthetic structures resident, cut them into --parts shards by id range
(fdgpu_index_split) --runs times, and for comparison do the same job the way the library offered before: --parts calls of fdgpu_index_remove
with range masks on the same resident index, in the same process.  Prints one JSON line with the per-stage device times (HIP events of
fdgpu_last_timings, not host clocks around asynchronous calls; medians over the runs), each stage's bytes moved / time, the split's rate against
the model 2 reads of V + 1 write of V, the sum of the removal calls, and a check that the merge of the parts is the source (byte for byte; above --full-check-bytes: sizes, posting
counts, sampled lists and every part verified with its own id range).

    python tools/split_probe.py [--structures 542000] [--parts 8] [--runs 3] [--seed 7]
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
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--full-check-bytes", type=int, default=4 << 30, help="compare the merged parts with the source byte for byte up to this many value bytes")
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
    bounds = indexio.shard_bounds(a.parts, a.structures)
    V, H = ix.value_len, ix.num_hashes
    ctx.enable_timing(True)
    split_runs, remove_runs, prune_runs = [], [], []
    ok = True
    for run in range(a.runs):
        got = ix.split(bounds)
        split_runs.append(timed())
        if run == 0:
            ctx.enable_timing(False)
            v_parts = sum(p.value_len for p in got)
            ok &= sum(p.num_postings for p in got) == ix.num_postings
            m = fd.FolddiscoIndexSet(got).merge()
            ok &= m.value_len == V and m.num_hashes == H
            if V <= a.full_check_bytes:
                ok &= all(np.array_equal(x, y) for x, y in zip(m.export_view(), ix.export_view()))
            else:                                 # two host copies of the value bytes are too much: sampled lists instead
                hs = np.random.Generator(np.random.PCG64(a.seed)).choice(got[a.parts // 2].export_view()[1], 64, replace=False).astype(np.uint32)
                ok &= all(np.array_equal(x, y) for x, y in zip(m.get_entries(hs), ix.get_entries(hs)))
                ok &= all(p.verify().ok for p in got)
            del m
            ctx.enable_timing(True)
        del got
        tot, stages = 0.0, {}
        for r in range(a.parts):                  # the same job with what the library had: one removal with a range mask per part
            keep = np.zeros(a.structures, bool)
            keep[int(bounds[r]): int(bounds[r + 1])] = True
            p = ix.remove(keep)
            t = timed()
            tot += sum(ms for ms, _ in t.values())
            for n, (ms, b) in t.items():
                s = stages.setdefault(n, [0.0, 0])
                s[0] += ms
                s[1] += b
            del p
        remove_runs.append(tot)
        prune_runs.append(stages)
    ctx.enable_timing(False)
    med = lambda xs: float(np.median(xs))
    names = list(split_runs[0])
    stage_ms = {n: round(med([r[n][0] for r in split_runs]), 3) for n in names}
    stage_gbps = {n: round(split_runs[0][n][1] / (stage_ms[n] * 1e-3) / 1e9, 1) if stage_ms[n] > 0 else None for n in names}
    split_ms = med([sum(ms for ms, _ in r.values()) for r in split_runs])
    model = 2 * V + v_parts
    pr = {n: round(med([r[n][1] for r in prune_runs]) / (med([r[n][0] for r in prune_runs]) * 1e-3) / 1e9, 1) for n in prune_runs[0] if med([r[n][0] for r in prune_runs]) > 0}
    out = dict(structures=a.structures, parts=a.parts, runs=a.runs, V=V, V_parts=v_parts, hashes=H, split_ms=round(split_ms, 3), split_stage_ms=stage_ms,
               split_stage_GBps=stage_gbps, split_model_GBps=round(model / (split_ms * 1e-3) / 1e9, 1),
               split_hbm_peak_fraction=round(model / (split_ms * 1e-3) / HBM_PEAK, 3), remove_calls_ms=round(med(remove_runs), 3),
               remove_stage_GBps=pr, speedup=round(med(remove_runs) / split_ms, 2), merge_check="pass" if ok else "FAIL")
    print(json.dumps(out), flush=True)
    return 0 if ok and split_ms < med(remove_runs) else 1


if __name__ == "__main__":
    sys.exit(main())
