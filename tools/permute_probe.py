"""Device cost of an index reorder at database scale: build --structures synthetic structures resident, permute the index with a seeded random
permutation and with the identity (fdgpu_index_permute) --runs times each.  Prints one JSON line with the per-stage device times (HIP events of
fdgpu_last_timings, not host clocks around asynchronous calls; medians over the runs), the rate of each call on the floor of DESIGN §4d (V read
twice, V' written once, 16 H bytes of tables) and a check that the permutation there and back is the source (byte for byte up to
--full-check-bytes; sizes, posting counts and the verdict of verify beyond).  Writes nothing.

    python tools/permute_probe.py [--structures 542000] [--runs 3] [--seed 7]
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--full-check-bytes", type=int, default=4 << 30, help="compare the index permuted there and back with the source byte for byte up to this many value bytes")
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
    S, V, H = a.structures, ix.value_len, ix.num_hashes
    perm = np.random.Generator(np.random.PCG64(a.seed)).permutation(S).astype(np.uint32)
    inv = np.empty(S, np.uint32)
    inv[perm.astype(np.int64)] = np.arange(S, dtype=np.uint32)
    ident = np.arange(S, dtype=np.uint32)
    ok = True
    got = ix.permute(perm)                        # the check, and the warm-up of the workspaces
    back = got.permute(inv)
    v_new = got.value_len
    ok &= got.num_postings == ix.num_postings == back.num_postings and got.num_hashes == H and back.value_len == V
    if V <= a.full_check_bytes:
        ok &= all(np.array_equal(x, y) for x, y in zip(back.export_view(), ix.export_view()))
    else:
        ok &= got.verify().ok and back.verify().ok
    del got, back
    ctx.enable_timing(True)
    runs = {"random": [], "identity": []}
    for _ in range(a.runs):
        for name, p in (("random", perm), ("identity", ident)):
            got = ix.permute(p)
            runs[name].append(timed())
            del got
    ctx.enable_timing(False)
    med = lambda xs: float(np.median(xs))
    out = dict(structures=S, runs=a.runs, V=V, V_permuted=v_new, hashes=H, round_trip_check="pass" if ok else "FAIL")
    for name, rs in runs.items():
        total = med([sum(ms for ms, _ in r.values()) for r in rs])
        floor = 2 * V + (v_new if name == "random" else V) + 16 * H
        out[name] = dict(ms=round(total, 3), stage_ms={n: round(med([r[n][0] for r in rs]), 3) for n in rs[0]}, floor_bytes=floor,
                         floor_GBps=round(floor / (total * 1e-3) / 1e9, 1), hbm_peak_fraction=round(floor / (total * 1e-3) / HBM_PEAK, 3))
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
