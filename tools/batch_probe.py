"""Device cost of the resident-batch operations at database scale: --structures synthetic structures resident as parts of one generated block
each, Batch.concat of the parts (8 at the default size), Batch.select of the whole with the identity and with a seeded random permutation, and — in
the same process, on the same stream — a plain device-to-device copy of the same five arrays, which is the yardstick: the gather moves every byte
once in and once out as the copy does, in runs of at most 768 bytes.  One warm-up, then --runs repetitions; device times are HIP events
(fdgpu_last_timings for the library's stages, torch events around the yardstick copies), medians.  Prints one JSON line; the select of the random
permutation is checked against a torch gather of the source.  Writes nothing.

    python tools/batch_probe.py [--structures 542000] [--runs 7] [--seed 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEN_BLOCK = 67750          # structures per generated block (bench.py's block): 542,000 structures are 8 parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=542000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--seed", type=int, default=7)
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

    blocks, parts = [], []
    for b in range(0, a.structures, GEN_BLOCK):
        d = synth.generate(min(GEN_BLOCK, a.structures - b), seed=a.seed + 1000 * (b // GEN_BLOCK), device=dev)
        blocks.append(d)
        parts.append(wrap(d))
    if len(parts) < 2:
        sys.exit("batch_probe: at least two blocks of %d structures are needed for the concat" % GEN_BLOCK)
    names = ("n_xyz", "ca_xyz", "cb_xyz", "aa")
    src = {k: torch.cat([d[k] for d in blocks]) for k in names}      # the yardstick's source, and the expectation of the check
    off = np.zeros(a.structures + 1, np.int64)
    off[1:] = np.cumsum(np.concatenate([np.diff(d["res_off"].cpu().numpy().astype(np.int64)) for d in blocks]))
    S, R = a.structures, int(off[-1])
    perm = np.random.Generator(np.random.PCG64(a.seed)).permutation(S)
    ident = np.arange(S)

    def stage(name):
        ctx.synchronize()
        return {n: ms for n, ms, _ in ctx.last_timings()}[name]

    def copy_ms():
        dst = {k: torch.empty_like(v) for k, v in src.items()}
        per = {}
        for k in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst[k].copy_(src[k])
            e1.record()
            e1.synchronize()
            per[k] = e0.elapsed_time(e1)
        return per

    whole = fd.Batch.concat(parts)                 # warm-up of every measured path, and the batch the selects read
    got = whole.select(perm)
    copy_ms()
    # check: the gathered arrays against a torch gather of the source
    lens = np.diff(off)[perm]
    idx = torch.from_numpy(np.repeat(off[:-1][perm] - (np.cumsum(lens) - lens), lens) + np.arange(R)).to(dev)
    ex = got.export()
    ok = all(bool((torch.from_numpy(getattr(ex, k)).to(dev).reshape(src[k].shape) == src[k][idx]).all()) for k in names)
    del ex, got, idx
    ctx.enable_timing(True)
    t = {"concat": [], "select_identity": [], "select_random": []}
    copies = []
    for _ in range(a.runs):
        c = fd.Batch.concat(parts)
        t["concat"].append(stage("batch_concat"))
        del c
        for name, ids in (("select_identity", ident), ("select_random", perm)):
            g = whole.select(ids)
            t[name].append(stage("batch_select"))
            del g
        copies.append(copy_ms())
    ctx.enable_timing(False)
    med = lambda xs: float(np.median(xs))
    copy = {k: round(med([c[k] for c in copies]), 3) for k in names}
    copy_total = med([sum(c.values()) for c in copies])
    moved = 2 * R * 37
    out = dict(structures=S, residues=R, parts=len(parts), runs=a.runs, bytes_moved=moved, gather_check="pass" if ok else "FAIL",
               copy_ms=round(copy_total, 3), copy_ms_per_array=copy, copy_GBps=round(moved / (copy_total * 1e-3) / 1e9, 1))
    for name, xs in t.items():
        out[name] = dict(ms=round(med(xs), 3), GBps=round(moved / (med(xs) * 1e-3) / 1e9, 1), times_the_copy=round(med(xs) / copy_total, 2))
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
