"""Device cost of an index update at database scale: build --structures synthetic structures resident, remove a seeded random --remove-frac
of them (fdgpu_index_remove), build --add new ones at the next ids and merge them in (fdgpu_index_merge).  Prints one JSON line with the
per-stage device times (HIP events of fdgpu_last_timings, not host clocks around asynchronous calls), V and V' (value bytes before / after the
prune), the prune's rate on (V + V') bytes and on the bytes it moves (2 V + V' + 8 per hash: two reads of V, one write of V'), and a
sampled check of the result.

    python tools/update_probe.py [--structures 542000] [--remove-frac 0.01] [--add 5420] [--seed 7]
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
    ap.add_argument("--remove-frac", type=float, default=0.01)
    ap.add_argument("--add", type=int, default=5420)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--samples", type=int, default=32)
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
        t = ctx.last_timings()
        return sum(ms for _, ms, _ in t), {n: round(ms, 3) for n, ms, _ in t}

    # the database: blocks built at consecutive first ids and merged on the device
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
    rng = np.random.Generator(np.random.PCG64(a.seed))
    keep = np.ones(a.structures, bool)
    keep[rng.choice(a.structures, int(round(a.remove_frac * a.structures)), replace=False)] = False
    ctx.enable_timing(True)
    pruned = ix.remove(keep)
    prune_ms, prune_stages = timed()
    new = wrap(synth.generate(a.add, seed=a.seed + 999_983, device=dev))
    part = fd.FolddiscoIndex.build(ctx, new, first_id=pruned.first_id + pruned.n_structures)
    build_ms, _ = timed()
    up = fd.FolddiscoIndexSet([pruned, part]).merge()
    merge_ms, merge_stages = timed()
    ctx.enable_timing(False)
    V, V2 = ix.value_len, pruned.value_len
    # sampled check: updated list == original list without the removed ids, the rest remapped, + the new part's ids
    _, h, _ = part.export()                   # the new part's hashes (small): lists that exist in the database as well, almost always
    hs = rng.choice(h, min(a.samples, len(h)), replace=False).astype(np.uint32)
    newid = np.cumsum(keep) - 1
    ok = True
    for q, old, got, add in zip(hs, ix.get_entries(hs), up.get_entries(hs), part.get_entries(hs)):
        want = np.concatenate([newid[old[keep[old]]], add]).astype(np.uint32)
        ok &= bool(np.array_equal(got, want))
    prune_bytes = 2 * V + V2 + 8 * ix.num_hashes
    out = dict(structures=a.structures, removed=int((~keep).sum()), added=a.add, V=V, V_pruned=V2, V_updated=up.value_len,
               hashes=ix.num_hashes, hashes_pruned=pruned.num_hashes, prune_ms=round(prune_ms, 3), prune_stages=prune_stages,
               prune_GBps=round((V + V2) / (prune_ms * 1e-3) / 1e9, 1),
               prune_hbm_peak_fraction=round((V + V2) / (prune_ms * 1e-3) / HBM_PEAK, 3),
               prune_moved_GBps=round(prune_bytes / (prune_ms * 1e-3) / 1e9, 1),
               new_part_build_ms=round(build_ms, 3), merge_ms=round(merge_ms, 3), merge_stages=merge_stages,
               device_update_ms=round(prune_ms + build_ms + merge_ms, 3), sampled_check="pass" if ok else "FAIL")
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
