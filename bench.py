#!/usr/bin/env python
"""bench.py — structures/sec indexed + motif queries/sec at Swiss-Prot scale on MI355X (BASELINE.json's metric).

Workload (config.workload): 542,000 synthetic AFDB-shaped structures in total (Swiss-Prot scale), generated in
eight fixed blocks of 67,750 (seed + 1000 * block) so that every --gpus N indexes the SAME database: rank r of N owns the
contiguous id range dist.shard_range(r, N, 542000) ("strong" scaling; index build shards by structure, no data-path
collective).

One step = the whole index build of the rank's shard, inputs resident in HBM: frames (residues in amino-acid order) ->
bucket counts -> pair emit (PDBTrRosetta hash, keys bucketed by the top six hash bits) -> three segmented 8-bit sort
passes -> delta/varint posting encode (fdgpu_index_build).  The whole shard is ONE call when its sort workspace fits the
device (12 B per key: 213 GB for Swiss-Prot on one MI355X); otherwise calls of 203,250 structures whose sub-indices are
merged on the device into ONE resident index (fdgpu_index_merge), byte-identical to a single build.
value = 542,000 * steps / time (max over ranks).

With --full, after the timed build: the export-inclusive rate (one more step + fdgpu_index_export D2H), the per-kernel HIP-event
timings of one step (roofline of the dominant kernel), the motif-query leg against the resident index (folddisco_amd/
querybench.py: queries/s, the scoring kernels' roofline and the oracle's count_query + retrieval on the host cores) and,
on rank 0 at N=1, the CPU restatement of the index build on a bounded sample.  Without --full those fields of the line are null:
a plain run generates the database, warms up, times the steps and prints the line.

--dump-outputs DIR: after the timed steps, rank 0 writes what its last timed step computed (the resident index of its shard as
fdgpu_index_export hands it to the host) as DIR/<name>.npy in float64 / float32, a fixed seeded sample of it (dump_outputs).

Contract: python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]  -> one JSON line on rank 0.  With N > 1 and
no WORLD_SIZE in the environment the script re-executes itself under torch.distributed.run (one rank per GPU, nccl = RCCL).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time
import threading

_WD_FIRED, _WD_LEFT, _WD_ARMED = threading.Event(), threading.Event(), []      # the N > 1 watchdog of main()

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
GEN_BLOCK = 67750      # structures per generated block = per fdgpu_index_build call (Swiss-Prot 542,000 / 8)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--structures", type=int, default=542000, help="structures in the WHOLE database (split over the ranks)")
    ap.add_argument("--seed", type=int, default=20260927)
    ap.add_argument("--cpu-sample", type=int, default=6144, help="structures timed on the host for cpu_baseline")
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-query", action="store_true")
    ap.add_argument("--no-export", action="store_true")
    ap.add_argument("--no-on-disk", action="store_true", help="skip the on-disk-inclusive step (index files written: one rank fdgpu_index_save, N ranks the device-side single index)")
    ap.add_argument("--build-chunk-blocks", type=int, default=0, help="0 (default): the rank's whole shard in ONE fdgpu_index_build call when its sort workspace fits the "
                    "device, else calls of 3 blocks.  N > 0: N generated blocks of 67,750 structures per call (3: 203,250 structures, ~6.7e9 keys; 1: as in rounds 1-2)")
    ap.add_argument("--no-cli-index", action="store_true", help="skip the drop-in `index` leg (20,500 structures as .pdb.gz files and as a Foldcomp database)")
    ap.add_argument("--no-replicas", action="store_true", help="skip the query-replica leg of --gpus N > 1 (index replicated, queries sharded)")
    ap.add_argument("--full", action="store_true", help="also run the legs behind the timed build (export / single-index / on-disk inclusive steps, per-kernel "
                    "roofline, motif queries, drop-in `index`, CPU baselines); the --no-* options above select among them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write a fixed seeded sample of the index the last timed step built to DIR/<name>.npy")
    return ap.parse_args()


DUMP_HASHES = 1 << 19       # --dump-outputs: posting lists sampled by position (hash, start offset, byte length of each)
DUMP_VALUE_BYTES = 1 << 21  # value bytes sampled by position
DUMP_IDS = 1 << 21          # decoded structure ids at most, from the first lists of the sample


def dump_outputs(ix, out_dir, seed):
    """--dump-outputs: the index the last timed step built, as a caller receives it from fdgpu_index_export (hashes u32[H], offsets u64[H+1]
    into the value bytes, value u8[]), plus the structure ids that fdgpu_get_entries decodes from some of its lists.  Swiss-Prot's index is
    26 GB: the arrays are sampled at positions drawn from `seed` (the same positions for the same index), ~36 MB of .npy in all.  Every
    value is an integer below 2^53, exact in float64 (value bytes: float32)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    v, h, o = ix.export_view()
    H, V = len(h), len(v)
    rng = np.random.default_rng(seed)
    pick = np.unique(rng.integers(0, H, DUMP_HASHES)) if H > DUMP_HASHES else np.arange(H)
    vpick = np.unique(rng.integers(0, V, DUMP_VALUE_BYTES)) if V > DUMP_VALUE_BYTES else np.arange(V)
    lens = ix.posting_lengths(h[pick]).astype(np.int64)
    n_dec = int(np.searchsorted(np.cumsum(lens), DUMP_IDS, side="right"))
    ids = ix.get_entries(h[pick[:n_dec]])
    out = {"index_counts": np.array([H, V, ix.num_postings, ix.n_structures, ix.first_id], np.float64),
           "hashes": h[pick].astype(np.float64), "offsets": o[pick].astype(np.float64), "list_bytes": (o[pick + 1] - o[pick]).astype(np.float64),
           "posting_lengths": lens.astype(np.float64), "value_bytes": v[vpick].astype(np.float32),
           "posting_ids": np.concatenate(ids).astype(np.float64) if ids else np.zeros(0, np.float64)}
    del v, h, o
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def respawn_under_torchrun(args):
    """python bench.py --gpus N with N > 1: start N ranks (one per GPU) over RCCL and hand them the same arguments"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.exit(subprocess.call(cmd, env=env))


def pmc_traffic(stage, tag):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes of this same command
    (profiles/*pmc_traffic_<tag>.json, tools/profile_bench.sh): 2 x FETCH_SIZE (gfx950 reports half of a coalesced stream,
    MI355X_MICROARCH.md; checked on k_enc_sizes / k_rs_hist whose read bytes are known) + WRITE_SIZE.  None when no profile
    of this workload is committed."""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", f"*pmc_traffic_{tag}.json")), reverse=True):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        for k, v in d.get("kernels", {}).items():
            if k.startswith("k_" + stage):
                return {"bytes_per_launch": 2.0 * v["fetch_bytes_per_launch"] + v["write_bytes_per_launch"], "kernel": k,
                        "rocprof_avg_us": v.get("avg_us"), "source": "committed PMC pass: profiles/" + os.path.basename(f),
                        "measured_in_this_run": False, "fetch_correction": 2.0}
    return None


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_budget():
    """cores this process may really use: the affinity mask and the cgroup CPU quota (a container can show 256 logical CPUs and grant far
    fewer; more OpenMP threads than that only add contention)"""
    info = {"logical_cpus": os.cpu_count() or 1}
    try:
        info["affinity"] = len(os.sched_getaffinity(0))
    except Exception:
        info["affinity"] = info["logical_cpus"]
    quota = None
    try:
        a, b = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        quota = None if a == "max" else float(a) / float(b)
    except Exception:
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            quota = q / per if q > 0 else None
        except Exception:
            quota = None
    info["cgroup_quota_cores"] = quota
    info["usable"] = max(1, int(min(info["affinity"], quota if quota else info["affinity"])))
    return info


def cpu_baseline_build(ps_sample, n_threads, fit_structs=0):
    """CPU restatement of the reference's index build (oracle/: OpenMP over structures for both hash passes like the reference's
    rayon par_iter, count/fill table build with the reference's `hash % T == tid` ownership partition), timed per stage on
    the host cores of this box.  fit_structs > 0: the table build is timed once more on the first fit_structs structures' lists — two
    sizes separate its fixed cost (the sweeps over the 2^30-entry tables, indextable.rs:204-295) from its per-posting cost."""
    import oracle
    from tests.helpers import packed_to_oracle_structs
    os.environ["OMP_NUM_THREADS"] = str(n_threads)
    structs = packed_to_oracle_structs(ps_sample)
    t0 = time.perf_counter()
    h, off = oracle.hash_batch(structs, n_threads=n_threads)        # pass 1 (collect_and_count, controller/mod.rs:274-365)
    t1 = time.perf_counter()
    h2, off2 = oracle.hash_batch(structs, n_threads=n_threads)      # pass 2 (add_entries, controller/mod.rs:367-441): the reference hashes twice
    t2 = time.perf_counter()
    oracle.build_index_from_lists_mt(h, off, n_threads)
    t3 = time.perf_counter()
    st = {"hash_pass1_s": t1 - t0, "hash_pass2_s": t2 - t1, "count_fill_finalize_s": t3 - t2}
    fit = None
    if fit_structs and fit_structs < len(structs):
        t4 = time.perf_counter()
        oracle.build_index_from_lists_mt(h[: int(off[fit_structs])], off[: fit_structs + 1], n_threads)
        t5 = time.perf_counter()
        n1, n0 = len(structs), fit_structs
        per = max(((t3 - t2) - (t5 - t4)) / (n1 - n0), 0.0)
        fit = {"table_build_s_at": {str(n1): t3 - t2, str(n0): t5 - t4}, "per_structure_s": per, "fixed_s": max((t3 - t2) - per * n1, 0.0)}
    return len(structs) / (t3 - t0), st, fit


def cli_index_leg(dev, seed, n_struct=20500):
    """The drop-in path a user runs (python -m folddisco_amd index, folddisco_amd/__main__.py): human-proteome scale, 20,500 synthetic
    structures written once as gzipped PDB files and once as a Foldcomp database (the reference's 24 fixture entries repeated), indexed end
    to end IN THIS PROCESS — multi-threaded native ingest double-buffered against the GPU builds, sub-indices merged on the device, one
    export, the four index files written.  Not the headline: real-format input is ingest-bound."""
    import shutil
    import tempfile
    import hashlib
    from folddisco_amd import synth
    from folddisco_amd import __main__ as cli
    work = tempfile.mkdtemp(prefix="fd_cli_bench_")
    # ingest threads sized from the cores this container is really granted (cgroup quota / affinity), not from the logical CPUs it can see: twice the
    # budget, at most 64 — measured on the 16-core quota of the GPU box: ingest 0.46 s with 16 threads, 0.41 with 32, 0.40 with 64 (the quota is
    # accounted per 100 ms period; a few more runnable threads than cores keep them busy across file boundaries).  FD_BENCH_INGEST_THREADS overrides.
    threads = int(os.environ.get("FD_BENCH_INGEST_THREADS", "0")) or max(1, min(64, 2 * cpu_budget()["usable"]))
    out = {"structures": n_struct, "ingest_threads": threads, "cpu_budget": cpu_budget()}
    try:
        d = synth.generate(n_struct, seed=seed + 77, device=dev)
        t0 = time.perf_counter()
        synth.write_pdb_gz(d, os.path.join(work, "pdb"), workers=min(64, os.cpu_count() or 1))
        out["write_inputs_s"] = round(time.perf_counter() - t0, 2)
        gz_bytes = sum(os.path.getsize(os.path.join(work, "pdb", f)) for f in os.listdir(os.path.join(work, "pdb")))
        legs = [("pdb_gz", os.path.join(work, "pdb"), gz_bytes)]
        fc_src = os.path.join(ROOT, "tests", "golden", "foldcomp", "example_db")
        if os.path.exists(fc_src):
            synth.replicate_foldcomp_db(fc_src, os.path.join(work, "db_foldcomp"), n_struct)
            legs.append(("foldcomp_db", os.path.join(work, "db_foldcomp"), os.path.getsize(os.path.join(work, "db_foldcomp"))))
        for name, src, nbytes in legs:
            import ctypes as _C
            from folddisco_amd import _lib as _fl
            for rep in range(2):            # the second run has the input in the page cache and the context's pools warm
                pre = os.path.join(work, "idx_%s_%d" % (name, rep))
                _fl.load().fdgpu_ingest_stats(None, 1)
                t0 = time.perf_counter()
                cli.main(["index", "-p", src, "-i", pre, "-t", str(threads), "--device", str(dev.index or 0)])
                wall = time.perf_counter() - t0
            T = dict(cli.LAST_TIMINGS)
            st5 = (_C.c_double * 5)()
            _fl.load().fdgpu_ingest_stats(st5, 0)        # thread-seconds of the ingest pool by stage (text input only)
            sha = hashlib.sha256(open(pre, "rb").read()).hexdigest()[:16]
            out[name] = {"value": n_struct / wall, "unit": "structures/s", "wall_s": round(wall, 3), "input_bytes": nbytes,
                         "ingest_s": round(T.get("ingest_s", 0.0), 3), "gpu_build_s": round(T.get("gpu_build_s", 0.0), 3), "device_merge_s": round(T.get("merge_s", 0.0), 3),
                         "export_and_files_s": round(T.get("export_write_s", 0.0), 3), "save_s": round(T.get("save_s", 0.0), 3), "chunks": T.get("chunks"), "index_bytes": os.path.getsize(pre),
                         "index_sha256_16": sha,
                         "ingest_thread_s": None if not st5[3] else {"read_inflate": round(st5[0], 3), "parse_text": round(st5[1], 3), "compact_build": round(st5[2], 3),
                                                                     "files": int(st5[3]), "inflated_bytes": int(st5[4]),
                                                                     "inflate_MB_per_s_per_thread": round(st5[4] / 1e6 / st5[0], 1) if st5[0] else None},
                         "note": "ingest runs on a host thread pool while the GPU builds the previous chunk: wall ~ ingest + last chunk + merge + export"}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return out


def cpu_baseline_query(ix, d, nres, res_off_h, qlist, top_n, match_top, S):
    """Query half of cpu_baseline: oracle/fdo_bench.c (the reference's make_query_map + count_query + sort/truncate + retrieval per
    query, OpenMP over queries where the reference uses rayon, query_pdb.rs:348) against the SAME index — the export of the
    resident index — on the host cores of this box."""
    import numpy as np
    import oracle
    v, h, o = ix.export_view()
    n_xyz, ca_xyz, cb_xyz, aa = (d[k].cpu().numpy() for k in ("n_xyz", "ca_xyz", "cb_xyz", "aa"))
    cores = cpu_budget()["usable"]
    reps = max(1, 2048 // max(len(qlist), 1))     # ~2,000 queries: seconds of CPU work on the granted cores
    r_all = oracle.query_bench(h, o, v, nres, res_off_h.astype(np.uint64), n_xyz, ca_xyz, cb_xyz, aa, qlist * reps, top_n=top_n,
                               match_top=match_top, n_threads=cores)
    r64 = oracle.query_bench(h, o, v, nres, res_off_h.astype(np.uint64), n_xyz, ca_xyz, cb_xyz, aa, qlist, top_n=top_n,
                             match_top=match_top, n_threads=min(64, cores))
    return {"value": len(qlist) * reps / r_all["wall_s"], "unit": "queries/s", "cores": cores, "kind": "port",
            "sample": "the same %d queries x%d against the export of the same resident index (%d structures): make_query_map + count_query + "
                      "sort/truncate %d + retrieval of the top %d, OpenMP over queries (query_pdb.rs:348), %.1f s wall" %
                      (len(qlist), reps, S, top_n, match_top, r_all["wall_s"]),
            "stage_thread_s": {k: round(x, 2) for k, x in r_all["stage_thread_s"].items()}, "matches": r_all["matches"] // reps,
            "t64": {"value": len(qlist) / r64["wall_s"], "cores": min(64, cores), "wall_s": round(r64["wall_s"], 2),
                    "stage_thread_s": {k: round(x, 2) for k, x in r64["stage_thread_s"].items()}}}


def PAR_NOTE(world):
    return "" if world == 1 else ("; the headline times INDEPENDENT shard builds (no data-path collective); single_index_inclusive = the same step + the hash-range "
                                  "exchange and per-range merge that make them one index")


def progress(msg):
    """FD_BENCH_TRACE=1: a line per leg on stderr (where a multi-rank run spends its time)"""
    if os.environ.get("FD_BENCH_TRACE"):
        print("[bench %s r%s] %s" % (time.strftime("%H:%M:%S"), os.environ.get("RANK", "0"), msg), file=sys.stderr, flush=True)


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_torchrun(args)
    import numpy as np
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1:
        import torch.distributed as dist  # noqa: F811
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        backend = os.environ.get("FD_BENCH_BACKEND", "nccl")   # "gloo": several ranks on ONE GPU (plumbing smoke test)
        if backend != "nccl":
            local_rank = local_rank % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import folddisco_amd as fd
    from folddisco_amd import synth
    from folddisco_amd.dist import shard_range

    S_total = args.structures
    lo, hi = shard_range(rank, world, S_total)
    S = hi - lo
    # ---- the rank's slice of the database, generated block by block directly in HBM
    blocks = []
    for b in range(lo // GEN_BLOCK, (hi - 1) // GEN_BLOCK + 1 if hi > lo else 0):
        g0 = b * GEN_BLOCK
        n_gen = min(GEN_BLOCK, S_total - g0)
        d = synth.generate(n_gen, seed=args.seed + 1000 * b, device=dev)
        a, e = max(lo, g0) - g0, min(hi, g0 + n_gen) - g0
        if a != 0 or e != n_gen:
            ro = d["res_off"]
            r0, r1 = int(ro[a]), int(ro[e])
            d = dict(res_off=(ro[a:e + 1] - ro[a]).contiguous(), n_xyz=d["n_xyz"][r0:r1].contiguous(), ca_xyz=d["ca_xyz"][r0:r1].contiguous(),
                     cb_xyz=d["cb_xyz"][r0:r1].contiguous(), aa=d["aa"][r0:r1].contiguous(), plddt=d["plddt"][r0:r1].contiguous())
        blocks.append(d)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev)
    ctx = fd.Context(local_rank, stream=stream.cuda_stream)

    def wrap(d):
        n = len(d["res_off"]) - 1
        ro = d["res_off"].contiguous()
        keep = (ro, d["n_xyz"], d["ca_xyz"], d["cb_xyz"], d["aa"])
        return ctx.wrap_device(n, int(ro[-1].item()), ro.data_ptr(), d["n_xyz"].data_ptr(), d["ca_xyz"].data_ptr(), d["cb_xyz"].data_ptr(),
                               d["aa"].data_ptr(), None, keepalive=keep)
    def cat_blocks(bs):
        if len(bs) == 1:
            return bs[0]
        out = {k: torch.cat([b[k] for b in bs]) for k in bs[0] if k != "res_off"}
        offs, base = [bs[0]["res_off"][:1]], 0
        for b in bs:
            offs.append(b["res_off"][1:] + base)
            base += int(b["res_off"][-1].item())
        out["res_off"] = torch.cat(offs).contiguous()
        return out
    # build calls: groups of consecutive blocks, one fdgpu_index_build each.  The MSD build holds 2^24 structures per call (6-byte sort elements:
    # 24 hash bits + 8 id bits in the key, 16 id bits beside it): the rank's whole shard goes into ONE call — no sub-indices, no merge — when
    # its 12 bytes of sort workspace per key fit the device next to the index (Swiss-Prot: 17.7e9 keys = 213 + 27 GB of 309), else into calls of
    # three blocks (203,250 structures).  --build-chunk-blocks N > 0 fixes the group size.
    R = sum(int(d["res_off"][-1].item()) for d in blocks)
    n_blocks = len(blocks)
    call_plan = {"blocks_per_call": None, "why": None}
    def est_one_call_bytes(res):
        keys = 104.0 * res          # postings per residue of the generator's AFDB-shaped structures: 101.2, + 3 %
        return keys * (12.0 + 1.6 + 0.13) + res * (80 + 14 + 16) + (6 << 30)
    if args.build_chunk_blocks > 0:
        g = max(1, min(args.build_chunk_blocks, (1 << 24) // GEN_BLOCK))
        call_plan.update(blocks_per_call=g, why="--build-chunk-blocks")
    else:
        torch.cuda.empty_cache()
        free_b, total_b = torch.cuda.mem_get_info(dev)
        need = est_one_call_bytes(R)
        ranks_here = max(1, world // max(torch.cuda.device_count(), 1)) if os.environ.get("FD_BENCH_BACKEND", "nccl") != "nccl" else 1
        g = n_blocks if (need < 0.97 * free_b / ranks_here and S <= (1 << 24)) else 3
        call_plan.update(blocks_per_call=g, why=f"auto: one call needs ~{need / 1e9:.0f} GB, {free_b / 1e9:.0f} GB free")
    def cat_groups(bl, g):
        return [cat_blocks(bl[k:k + g]) for k in range(0, len(bl), g)]
    def split_groups(d, per):
        """the inverse of cat_blocks: views of `per` structures each (the fall-back when the one-call build does not fit)"""
        out, n = [], len(d["res_off"]) - 1
        for a in range(0, n, per):
            e = min(n, a + per)
            ro = d["res_off"]
            r0, r1 = int(ro[a]), int(ro[e])
            R = int(ro[-1])
            part = {}
            for k, v in d.items():       # per-residue fields by residue range, per-structure fields by structure range: anything else is a bug here
                if k == "res_off":
                    part[k] = (ro[a:e + 1] - ro[a]).contiguous()
                elif len(v) == R:
                    part[k] = v[r0:r1]
                elif len(v) == n:
                    part[k] = v[a:e]
                else:
                    raise ValueError("split_groups: field %r has %d entries (residues %d, structures %d)" % (k, len(v), R, n))
            out.append(part)
        return out
    blocks = cat_groups(blocks, max(g, 1))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    chunk_batches = [wrap(d) for d in blocks]
    CALL_MAX = max((len(d["res_off"]) - 1 for d in blocks), default=0)

    def build_shard():
        """the rank's whole index: one build call per block, then the device merge into ONE resident index"""
        parts, fid = [], lo
        for cb in chunk_batches:
            parts.append(fd.FolddiscoIndex.build(ctx, cb, first_id=fid))
            fid += cb.n_struct
        if len(parts) == 1:
            return parts[0]
        return fd.FolddiscoIndexSet(parts).merge()

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    def max_over_ranks(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def sum_over_ranks(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return float(t.item())

    progress("database generated, build starts")
    ix = None
    if len(chunk_batches) == 1 and n_blocks > 3 and args.build_chunk_blocks <= 0:
        # the one-call plan is an estimate: a device that cannot hold it answers the first build with FDGPU_EHIP (hipMalloc), not with a crash —
        # then the workspaces go back and the shard is built in calls of three blocks, as in round 3's first half
        try:
            if os.environ.get("FD_BENCH_TEST_FALLBACK"):      # exercises the fall-back without needing a device that is too small
                raise fd.FdgpuError("forced by FD_BENCH_TEST_FALLBACK")
            ix = build_shard()
        except fd.FdgpuError as e:
            progress(f"one-call build did not fit ({e}); falling back to calls of three blocks")
            ix = None
            ctx.release_workspaces()
            chunk_batches = None
            blocks = split_groups(blocks[0], 3 * GEN_BLOCK)
            chunk_batches = [wrap(d) for d in blocks]
            CALL_MAX = max((len(d["res_off"]) - 1 for d in blocks), default=0)
            call_plan.update(blocks_per_call=3, why=call_plan["why"] + "; one-call build failed: " + str(e)[:200])
    for _ in range(args.warmup):
        ix = None
        ix = build_shard()
    ctx.synchronize()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ix = None  # release the previous index before building the next one
        ix = build_shard()
    ctx.synchronize()
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    value = S_total * args.steps / dt
    n_post, n_hash, vlen = ix.num_postings, ix.num_hashes, ix.value_len
    if args.dump_outputs and rank == 0:
        dump_outputs(ix, args.dump_outputs, args.seed)
    R_tot, post_tot, vlen_tot, hash_tot = (sum_over_ranks(x) for x in (R, n_post, vlen, n_hash))

    progress("timed build done")
    # ---- N > 1: the legs behind this point (single index over ncclSend / ncclRecv, sharded queries with RCCL exchanges, replicas) run collectives that no
    # machine with fewer than N GPUs can have executed; a rank that waits in one of them for ever would take the measured headline with it.  A watchdog
    # per rank therefore bounds them: when FD_BENCH_WATCHDOG_S (default 1500 s, 0 = off) pass behind the timed build without the line being printed, rank 0
    # prints the line with the legs that did finish (and says so under "watchdog"), and every rank leaves.  One rank (N = 1) has no watchdog.
    import threading
    wd_done, wd_printed = threading.Event(), threading.Event()
    wd_limit = float(os.environ.get("FD_BENCH_WATCHDOG_S", "1500")) if world > 1 else 0.0

    def partial_line():
        def got(fn):
            try:
                return fn()
            except NameError:       # the leg had not started when the watchdog fired
                return None
        return {"metric": "structures/sec indexed", "value": value, "unit": "structures/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32+u32", "data": "synthetic",
                "config": {"workload": f"Swiss-Prot scale: {S_total} synthetic AFDB-shaped structures index build, PDBTrRosetta default; {world} rank(s), contiguous id ranges",
                           "structures": S_total, "structures_per_gpu": S, "parallelism": f"shard-by-structure x{world}" + PAR_NOTE(world)},
                "roofline": got(lambda: roofline), "export_inclusive": got(lambda: export), "single_index_inclusive": got(lambda: single_index),
                "index_on_disk_inclusive": got(lambda: on_disk), "cpu_baseline": None,
                "query": got(lambda: query), "cli_index": None}

    def watchdog():
        if wd_done.wait(wd_limit):
            return
        _WD_FIRED.set()
        if rank == 0 and not wd_printed.is_set():
            line = partial_line()
            line["watchdog"] = {"fired_after_s": wd_limit, "note": "a leg behind the timed build did not return on some rank; value / ms_per_step are the completed "
                                                                    "measurement, legs that are null or partial did not finish"}
            try:
                print(json.dumps(line), flush=True)
            except Exception:  # noqa: BLE001 — a leg's half-built dictionary must not cost the headline
                for k in ("roofline", "export_inclusive", "single_index_inclusive", "index_on_disk_inclusive", "query"):
                    line[k] = None
                print(json.dumps(line), flush=True)
        _WD_LEFT.set()
        os._exit(0)      # every rank leaves within milliseconds of the others (the limit counts from the barrier behind the timed build)
    if wd_limit > 0:
        _WD_ARMED.append(True)
        threading.Thread(target=watchdog, daemon=True).start()
    # ---- export-inclusive: one more step that also brings the index to the host in the on-disk layout (fdgpu_index_export)
    export = None
    if args.full and not args.no_export:
        import ctypes as C
        from folddisco_amd._lib import u8p, u32p, u64p
        ix = None
        barrier()
        t0e = time.perf_counter()
        ix = build_shard()
        vp, hp, op = u8p(), u32p(), u64p()
        vl, H = C.c_uint64(), C.c_uint64()
        ctx.check(ctx.L.fdgpu_index_export(ctx.h, ix.h, C.byref(vp), C.byref(vl), C.byref(hp), C.byref(op), C.byref(H)))
        t1e = time.perf_counter()
        for p in (vp, hp, op):
            ctx.L.fdgpu_free(p)
        barrier()
        dte = max_over_ranks(t1e - t0e)
        export = {"value": S_total / dte, "unit": "structures/s", "ms_per_step": dte * 1e3, "bytes_to_host_per_rank": int(vl.value + 12 * H.value + 8),
                  "note": "one step + fdgpu_index_export (D2H of value bytes, hashes, offsets into malloc'd host buffers)"}

    # ---- N > 1, single-index inclusive: one more step that ends with ONE index of the whole database spread over the ranks by hash range (what
    # `folddisco index` must produce: SURVEY §8e row 2) — the timed shard build + hash bounds of equal posting bytes from rank 0 + piece j of every
    # rank's sub-index to rank j (ncclSend / ncclRecv under nccl; host objects under gloo) + per-range device merge.  NO file I/O.  The headline
    # above times independent shard builds and contains no exchange: this is the number that does.  Expected bytes leaving a rank:
    # (its value bytes + 12 B per hash) x (N - 1) / N.
    single_index = None
    if args.full and world > 1 and not args.no_export:
        try:
            from folddisco_amd import dist as fdist
            comm_si = fdist.Comm(ctx, rank, world) if dist.get_backend() == "nccl" else None
            ix = None
            barrier()
            t0s = time.perf_counter()
            ix = build_shard()
            sent = int((ix.value_len + 12 * ix.num_hashes) * (world - 1) / world)
            rng, hb_, vb_, ht_, vt_ = comm_si.single_index(ix) if comm_si is not None else fdist.single_index_over_process_group(ctx, ix)
            ctx.synchronize()
            t1s = time.perf_counter()
            barrier()
            dts = max_over_ranks(t1s - t0s)
            held = (rng.num_hashes, rng.value_len)
            rng = None
            comm_si = None
            single_index = {"value": S_total / dts, "unit": "structures/s", "ms_per_step": dts * 1e3, "exchange_bytes_sent_by_rank0_estimate": sent,
                            "total_hashes": int(ht_), "total_value_bytes": int(vt_), "rank0_range_hashes": int(held[0]), "rank0_range_value_bytes": int(held[1]),
                            "transport": "ncclSend / ncclRecv, device to device" if dist.get_backend() == "nccl" else "torch.distributed objects over gloo (host staging: not the RCCL path)",
                            "note": "one step + fdgpu_comm_single_index (bounds, slices, exchange, per-range merge), no files; max over ranks"}
        except Exception as e:  # noqa: BLE001 — the headline line must still be printed
            single_index = {"error": repr(e)[:300]}
        progress("single-index leg done")

    # ---- on-disk inclusive: one more step that ends with the reference's PREFIX / PREFIX.offset on a file system.  One rank: fdgpu_index_save (device
    # arrays streamed through pinned slots into pwrite).  N ranks: the single index without the host (Option A; csrc/fd_shard_index.hip):
    # hash ranges of equal posting bytes, piece j of every rank's sub-index to rank j (ncclSend / ncclRecv under nccl), per-range device merge, every rank
    # writes its regions of the two files.  Never `value`.
    on_disk = None
    if args.full and not args.no_export and not args.no_on_disk:
        import shutil
        import tempfile
        try:
            from folddisco_amd import dist as fdist
            need = int(vlen * 1.02 + 12.5 * n_hash) * (world if world > 1 else 1) + (1 << 20)
            cands = [d for d in (os.environ.get("FD_BENCH_DISK_DIR"), "/dev/shm", tempfile.gettempdir()) if d and os.path.isdir(d)]
            best = max(cands, key=lambda d: shutil.disk_usage(d).free)
            box = [None]
            if rank == 0 and shutil.disk_usage(best).free > 1.25 * need:
                box[0] = tempfile.mkdtemp(prefix="fd_bench_index_", dir=best)
            if dist is not None:
                dist.broadcast_object_list(box, src=0, device=dev if dist.get_backend() == "nccl" else None)
            if box[0] is None:
                on_disk = {"skipped": "no directory with %.1f GB free (tried %s)" % (1.25 * need / 1e9, ", ".join(cands))}
            else:
                prefix = os.path.join(box[0], "bench_folddisco")
                comm_ix = fdist.Comm(ctx, rank, world) if (dist is not None and dist.get_backend() == "nccl") else None
                ix = None
                barrier()
                t0d = time.perf_counter()
                ix = build_shard()
                if dist is None:
                    ix.save(prefix)
                    ht, vt = ix.num_hashes, ix.value_len
                else:
                    rng, hb, vb, ht, vt = comm_ix.single_index(ix) if comm_ix is not None else fdist.single_index_over_process_group(ctx, ix)
                    rng.save_part(prefix, hb, vb, ht, vt, write_header=(rank == 0), is_last=(rank == world - 1))
                    rng = None
                ctx.synchronize()
                barrier()
                dtd = max_over_ranks(time.perf_counter() - t0d)
                if rank == 0:
                    sz = (os.path.getsize(prefix), os.path.getsize(prefix + ".offset"))
                    on_disk = {"value": S_total / dtd, "unit": "structures/s", "ms_per_step": dtd * 1e3, "file_bytes": sz[0] + sz[1], "directory": best,
                               "files_complete": bool(sz[0] == vt and sz[1] == 8 + 4 * ht + 8 * (ht + 1)),
                               "note": ("one step + fdgpu_index_save: PREFIX and PREFIX.offset written from the device arrays" if dist is None else
                                        "one step + the single index of all ranks WITHOUT the host: hash ranges, piece j of every rank to rank j (%s), per-range device "
                                        "merge, every rank writes its regions of PREFIX / PREFIX.offset" % ("ncclSend / ncclRecv" if comm_ix is not None else "torch.distributed objects: gloo has no device path"))}
                comm_ix = None
                barrier()
                if rank == 0:
                    shutil.rmtree(box[0], ignore_errors=True)
        except Exception as e:  # noqa: BLE001 — the headline line must still be printed
            on_disk = {"error": repr(e)[:300]}

    # ---- per-kernel timings of one more (untimed) step with HIP events on the build stream -> roofline
    roofline = None
    if args.full:
        ctx.enable_timing(True)
        ix = None
        stages, parts, fid = [], [], lo
        for cb in chunk_batches:
            parts.append(fd.FolddiscoIndex.build(ctx, cb, first_id=fid))
            ctx.synchronize()
            stages += ctx.last_timings()
            fid += cb.n_struct
        if len(parts) > 1:
            ix = fd.FolddiscoIndexSet(parts).merge()
            ctx.synchronize()
            stages += ctx.last_timings()
        else:
            ix = parts[0]
        parts = None
        ctx.enable_timing(False)
        agg = {}
        for name, ms, by in stages:
            a = agg.setdefault(name, [0.0, 0, 0])
            a[0] += ms; a[1] += by; a[2] += 1
        dom_name, (dom_ms, dom_bytes, dom_n) = max(agg.items(), key=lambda kv: kv[1][0])
        achieved = dom_bytes / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0
        tag = f"S{S_total}" if world == 1 else f"S{S_total}_N{world}"
        tr = pmc_traffic(dom_name, tag)
        if tr and dom_n and not (0.5 < tr["bytes_per_launch"] / (dom_bytes / dom_n) < 2.0):
            tr = None      # the committed PMC passes are of another call plan (launch sizes differ): no traffic figure rather than a wrong one
        b_idx = 37.0 * R_tot / S_total + 8.0 * post_tot / S_total + vlen_tot / S_total + 12.0 * hash_tot / S_total
        roofline = {"bound": "hbm", "kernel": dom_name, "launches_per_step": dom_n, "avg_ms": dom_ms / max(dom_n, 1),
                    "algorithmic_bytes_per_launch": dom_bytes / max(dom_n, 1),
                    "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                    "traffic": tr["bytes_per_launch"] if tr else None, "traffic_detail": tr,
                    # SURVEY §8(d) end-to-end figure: B_idx = 37 R + 4 U + 4 U + v U + 12 H/S bytes per structure, per GPU
                    "end_to_end": {"algorithmic_bytes_per_structure": b_idx, "achieved": value / world * b_idx / 1e9, "unit": "GB/s",
                                   "frac": value / world * b_idx / 1e9 / HBM_PEAK_GBS},
                    "stages_ms": {k: round(v[0], 3) for k, v in agg.items()},
                    "stages_gbs": {k: round(v[1] / (v[0] * 1e-3) / 1e9, 1) if v[0] > 0 else 0.0 for k, v in agg.items()}}

    n_calls = len(chunk_batches)
    if n_calls == 1 and n_blocks > 3:
        ctx.release_workspaces()      # 213 GB of sort buffers: not needed by the legs that follow
    progress("stage timings done, query leg starts")
    # ---- motif queries against the resident index of the shard
    query = None
    if args.full and not args.no_query:
        try:
            from folddisco_amd import querybench
            d_all = {k: (torch.cat([b[k] for b in blocks]) if k != "res_off" else None) for k in blocks[0]}
            offs, base = [blocks[0]["res_off"][:1]], 0
            for b in blocks:
                offs.append(b["res_off"][1:] + base)
                base += int(b["res_off"][-1].item())
            d_all["res_off"] = torch.cat(offs).contiguous()
            chunk_batches = None
            blocks = None
            db = wrap(d_all)
            query = querybench.run(ctx, db, ix, d_all, S, world, rank, dist, dev, n_queries=args.queries, lo=lo, S_total=S_total,
                                   cpu_baseline_fn=cpu_baseline_query if (rank == 0 and world == 1 and not args.no_cpu_baseline) else None)
        except Exception as e:  # the index-build line must still be printed
            import traceback
            query = {"error": repr(e), "trace": traceback.format_exc()[-1500:]}
        progress("query leg done")
        # ---- query replicas (SURVEY §8e last row): every rank builds the WHOLE index (26 GB of 288) and the queries are dealt to the ranks
        if world > 1 and not args.no_replicas and query is not None and "error" not in query:
            try:
                ix = None; db = None; d_all = None
                torch.cuda.empty_cache()
                fblocks = [synth.generate(min(GEN_BLOCK, S_total - g0), seed=args.seed + 1000 * (g0 // GEN_BLOCK), device=dev) for g0 in range(0, S_total, GEN_BLOCK)]
                parts, fid = [], 0
                for fb in fblocks:
                    wb = wrap(fb)
                    parts.append(fd.FolddiscoIndex.build(ctx, wb, first_id=fid))
                    fid += wb.n_struct
                ixf = parts[0] if len(parts) == 1 else fd.FolddiscoIndexSet(parts).merge()
                parts = None
                d_full = {k: (torch.cat([b[k] for b in fblocks]) if k != "res_off" else None) for k in fblocks[0]}
                offs, base = [fblocks[0]["res_off"][:1]], 0
                for b in fblocks:
                    offs.append(b["res_off"][1:] + base)
                    base += int(b["res_off"][-1].item())
                d_full["res_off"] = torch.cat(offs).contiguous()
                fblocks = None
                progress("replica index built")
                query["replicas"] = querybench.run_replicas(ctx, wrap(d_full), ixf, d_full, S_total, world, rank, dist, dev, n_queries=args.queries)
                # N > 1: the headline is the better of the two multi-GPU forms, named — the sharded index (one query set scored by all ranks, RCCL
                # exchange) and the replicas (whole index per rank, queries dealt out; the form that scales for batches)
                rep = query["replicas"]
                query["sharded_value"] = query.get("value")
                if isinstance(rep, dict) and rep.get("value") and rep["value"] > (query.get("value") or 0.0):
                    query["value"] = rep["value"]; query["ms_per_query"] = rep.get("ms_per_query"); query["value_from"] = "replicas"
                else:
                    query["value_from"] = "sharded"
            except Exception as e:
                import traceback
                query["replicas"] = {"error": repr(e), "trace": traceback.format_exc()[-1500:]}

    cli_index = None
    if args.full and rank == 0 and world == 1 and not args.no_cli_index:
        try:
            ix = None; db = None
            torch.cuda.empty_cache()
            cli_index = cli_index_leg(dev, args.seed)
        except BaseException as e:  # noqa: BLE001 — sys.exit inside the CLI included: the bench line must still be printed
            cli_index = {"error": repr(e)}
    if rank == 0:
        cpu = None
        if args.full and world == 1 and not args.no_cpu_baseline:
            d0 = d_all if query is not None and "error" not in query else synth.generate(min(GEN_BLOCK, S_total), seed=args.seed, device=dev)
            ns = min(args.cpu_sample, len(d0["res_off"]) - 1)
            off = d0["res_off"][: ns + 1].cpu().numpy().astype(np.uint64)
            r_s = int(off[-1])
            ps = fd.PackedStructures(off, d0["n_xyz"][:r_s].cpu().numpy(), d0["ca_xyz"][:r_s].cpu().numpy(), d0["cb_xyz"][:r_s].cpu().numpy(),
                                     d0["aa"][:r_s].cpu().numpy())
            budget = cpu_budget()
            cores = budget["usable"]
            nq4 = ns // 4
            v_all, st_all, fit = cpu_baseline_build(ps, cores, fit_structs=nq4)
            ps64 = fd.PackedStructures(off[: nq4 + 1], ps.n_xyz[: int(off[nq4])], ps.ca_xyz[: int(off[nq4])], ps.cb_xyz[: int(off[nq4])], ps.aa[: int(off[nq4])])
            v64, st64, _ = cpu_baseline_build(ps64, 64)
            # what the sample says about the metric's own size: hashing is linear in the structures, the table build is its fixed sweeps + a
            # per-structure cost (two sizes measured) — an EXTRAPOLATION, labelled as one, because a bounded sample cannot amortise the sweeps
            hash_per = (st_all["hash_pass1_s"] + st_all["hash_pass2_s"]) / ns
            extr = None
            if fit:
                t_full = hash_per * S_total + fit["fixed_s"] + fit["per_structure_s"] * S_total
                extr = {"structures": S_total, "value": S_total / t_full, "unit": "structures/s", "seconds": t_full,
                        "hashing_s": hash_per * S_total, "table_fixed_s": fit["fixed_s"], "table_per_structure_s": fit["per_structure_s"],
                        "note": "extrapolated from the sample's stage times, not measured: 2 x hashing linear in the structures + table build = fixed "
                                "sweeps of the 2^30-entry tables + per-structure cost fitted on two sample sizes"}
            rate_all = ns / (st_all["hash_pass1_s"] + st_all["hash_pass2_s"]) * 2
            rate_64 = nq4 / (st64["hash_pass1_s"] + st64["hash_pass2_s"]) * 2
            cpu = {"value": v_all, "unit": "structures/s", "cores": cores, "cpu_model": cpu_model(), "cpu_budget": budget, "kind": "port",
                   "sample": f"first {ns} structures of the database ({r_s} residues): 2x hash+sort+dedup (OpenMP over structures) + count/fill "
                             f"table build with the reference's ownership partition, {cores} threads, {sum(st_all.values()):.1f} s; the table build's fixed "
                             f"2^30-entry sweeps are {100.0 * (fit['fixed_s'] if fit else 0.0) / max(sum(st_all.values()), 1e-9):.0f} % of it "
                             f"(extrapolated_to_metric_size puts the sample's stage costs at {S_total} structures)",
                   "stages_s": {k: round(v, 2) for k, v in st_all.items()}, "table_build_fit": fit, "extrapolated_to_metric_size": extr,
                   "hashing_structures_per_s": {"threads_%d" % cores: rate_all, "threads_64": rate_64, "scaling": rate_all / rate_64 if rate_64 > 0 else None,
                                                "note": "hashing is embarrassingly parallel over structures (per-thread scratch, no allocation per structure, longest "
                                                        "structures first); where %d threads do not beat 64 the box grants this container fewer cores than it shows "
                                                        "(cpu_budget) or its SMT siblings share the FP units" % cores},
                   "t64": {"value": v64, "cores": 64, "sample": f"first {nq4} structures, 64 threads (README's -t 64), {sum(st64.values()):.1f} s",
                           "stages_s": {k: round(v, 2) for k, v in st64.items()}}}
        out = {
            "metric": "structures/sec indexed", "value": value, "unit": "structures/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32+u32", "data": "synthetic", "full": args.full,
            "config": {"workload": f"Swiss-Prot scale: {S_total} synthetic AFDB-shaped structures ({int(R_tot)} residues, {int(post_tot)} postings, "
                                   f"{int(vlen_tot)} value bytes) index build, PDBTrRosetta default; {world} rank(s), contiguous id ranges, "
                                   f"per rank {n_calls} build call(s) of <= {CALL_MAX} structures" + (" merged on the device into one resident index" if n_calls > 1 else ": one resident index, no merge"),
                       "structures": S_total, "structures_per_gpu": S, "residues": int(R_tot), "postings": int(post_tot),
                       "parallelism": f"shard-by-structure x{world}" + PAR_NOTE(world), "build_calls_per_rank": n_calls, "call_plan": call_plan},
            "roofline": roofline, "export_inclusive": export, "single_index_inclusive": single_index, "index_on_disk_inclusive": on_disk, "cpu_baseline": cpu,
            "query": query, "cli_index": cli_index,
        }
        print(json.dumps(out), flush=True)
        wd_printed.set()
    if dist is not None:
        dist.barrier()      # (still under the watchdog: a rank that never arrives must not keep the others here)
        wd_done.set()
        dist.destroy_process_group()
    wd_done.set()


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        # N > 1 under the watchdog: a rank whose peers have just left through it sees its collective fail ("connection closed by peer") a moment before
        # its own limit — that is the watchdog's exit, not an error of this rank
        if _WD_ARMED and _WD_FIRED.wait(10.0):
            _WD_LEFT.wait(30.0)
            os._exit(0)
        raise
