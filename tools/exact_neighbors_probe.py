"""Device cost of the exact neighbours (fdgpu_rowset_neighbors) on the synthetic index of --structures structures (as tools/overlap_probe.py
builds it).  Per --sizes entry Q: the rows of Q seeded distinct structures spread over the whole index are kept in a row set and their
--k nearest structures of the whole index selected — HIP events of fdgpu_last_timings summed per stage over the blocks (xn_upload, xn_count,
xn_select, xn_merge, xn_copy), one warm-up, medians of --runs.  Reported with them: the postings walked (the lengths of the lists of every
query hash, summed: one counter add each) and that figure over the xn_count time; the host form (fdgpu_rows_neighbors_host on --host-threads
threads) with a check that it equals the device byte for byte; and, on the smallest size only, the only exact route there was before:
indexio.row_overlaps over --before-queries x S pairs (every row of the index extracted, every query row read S times), in the same process,
with its time per query against the new one's.

Every size is a child process of its own (it builds the index, measures, and ends) under its own time limit; the first one that fails ends
the probe.  One JSON line, also written to --out if given.

    python tools/exact_neighbors_probe.py [--structures 67750] [--sizes 256 4096] [--out profiles/exact_neighbors_probe_S67750.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def step_size(a):
    from folddisco_amd import indexio
    from overlap_probe import build_index, stages
    ctx, ix = build_index(a)
    S = a.structures
    rng = np.random.Generator(np.random.PCG64(a.seed))
    ids = np.sort(rng.choice(S, size=min(a.n, S), replace=False))
    d_len = np.ascontiguousarray(ix.signatures()["n"], dtype=np.uint32)
    ex = ids.astype(np.uint32)
    med = lambda xs: float(np.median(xs))
    Q, taken = ix.rowset(ids, window=a.window)
    assert taken == len(ids)
    rows = Q.export()
    postings = int(ix.posting_lengths(rows[0]).sum())
    got = np.array(ctx.rowset_neighbors(Q, ix, d_len, k=a.k, exclude=ex))      # the warm-up of the workspaces
    ctx.enable_timing(True)
    runs = []
    for _ in range(a.runs):
        again = ctx.rowset_neighbors(Q, ix, d_len, k=a.k, exclude=ex)
        runs.append(stages(ctx))
    ctx.enable_timing(False)
    ok = again.tobytes() == got.tobytes()
    ms = {k: round(med([r.get(k, 0.0) for r in runs]), 3) for k in runs[0]}
    files = ix.export() + (S, 0)
    hq = min(len(ids), a.host_queries)               # the host form on a prefix of the queries, its time scaled to all of them
    t0 = time.perf_counter()
    want = indexio.rows_neighbors_host((rows[0][:int(rows[1][hq])], rows[1][:hq + 1]), files, d_len, k=a.k, exclude=ex[:hq], threads=a.host_threads)
    host_s = (time.perf_counter() - t0) * len(ids) / hq
    got_h = got[:hq]
    ok &= want.tobytes() == got_h.tobytes()
    total_ms = sum(ms.values())
    out = dict(queries=len(ids), k=a.k, V=ix.value_len, hashes=ix.num_hashes, postings=ix.num_postings, query_hashes=int(Q.n_hashes), postings_walked=postings,
               stage_ms=ms, total_ms=round(total_ms, 3), xn_count_postings_per_s=round(postings / max(ms.get("xn_count", 0.0), 1e-6) * 1e3, 0),
               xn_count_add_GBps=round(4 * postings / max(ms.get("xn_count", 0.0), 1e-6) / 1e6, 2), host_form_s=round(host_s, 3), host_threads=a.host_threads,
               host_queries=hq, host_over_device=round(host_s / max(total_ms * 1e-3, 1e-9), 1), host_equals_device=bool(want.tobytes() == got_h.tobytes()))
    if a.yardstick:                                  # the route before: all Q x S pairs through the pair intersect
        nq = min(a.before_queries, len(ids))
        qa, qb = np.repeat(ids[:nq], S), np.tile(np.arange(S, dtype=np.int64), nq)
        t0 = time.perf_counter()
        inter, n_a, n_b = indexio.row_overlaps(ix, None, qa, qb, window=a.window)
        before_s = time.perf_counter() - t0
        inter = np.asarray(inter).reshape(nq, S)
        same = all(int(inter[q, int(r["id"])]) == int(r["inter"]) for q in range(nq) for r in got[q] if int(r["id"]) != indexio.ROW_NO_ID)
        ok &= same
        out["route_before"] = dict(queries=nq, pairs=int(nq * S), row_overlaps_s=round(before_s, 3), s_per_query=round(before_s / nq, 4), equals_device=bool(same))
        out["before_over_now_per_query"] = round((before_s / nq) / max(total_ms * 1e-3 / len(ids), 1e-12), 1)
    Q.close()
    out["ok"] = bool(ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=67750)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 4096], help="numbers of distinct query structures")
    ap.add_argument("-k", type=int, default=8)
    ap.add_argument("--window", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--before-queries", type=int, default=4, help="queries the route before is timed on (x S pairs)")
    ap.add_argument("--host-queries", type=int, default=512, help="queries the host form is timed on (its time is scaled to all of them)")
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
    out, ok = dict(structures=a.structures, k=a.k, window=a.window, runs=a.runs, host_threads=a.host_threads), True
    common = [sys.executable, os.path.abspath(__file__), "--structures", str(a.structures), "--seed", str(a.seed), "--runs", str(a.runs), "-k", str(a.k),
              "--host-threads", str(a.host_threads), "--window", str(a.window), "--before-queries", str(a.before_queries), "--host-queries", str(a.host_queries)]
    steps = [(f"queries_{n}", ["--step", "size", "--n", str(n)] + (["--yardstick"] if n == min(a.sizes) else [])) for n in a.sizes]
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
