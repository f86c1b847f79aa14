"""`python -m folddisco_amd index|query|update|verify|rows|dups|reshard|merge|reorder|coords …` — the reference's two hot-path subcommands (and `update`, `verify`, `rows`, `dups`, `reshard`, `merge`, `reorder` and `coords`, which it lacks) with its flag names and defaults
(src/cli/main.rs:26-110, src/cli/workflows/build_index.rs:64-241, src/cli/workflows/query_pdb.rs:144-519), driving the
GPU path through the C ABI.  Structure order = lexicographic path order (the reference uses readdir order, which is
filesystem dependent; SURVEY §7 hard part 3).  Only the default PDBTrRosetta encoding is supported; input is PDB or mmCIF, optionally gzip."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from folddisco_amd._lib import HASH_TYPE_NAMES, hash_type_index, parse_multiple_bins


def _load_paths(d: str, recursive: bool):
    out = []
    if os.path.isfile(d):
        return [d]
    for root, dirs, files in os.walk(d):
        for f in files:
            if f.lower().endswith((".pdb", ".ent", ".pdb.gz", ".ent.gz", ".cif", ".cif.gz", ".mmcif", ".mmcif.gz")):
                out.append(os.path.join(root, f))
        if not recursive:
            break
    return sorted(out)


def _init_dist(a):
    """torchrun / torch.distributed.run launch: one rank per GPU (backend nccl = RCCL; FD_BENCH_BACKEND=gloo puts several ranks on one
    GPU for plumbing tests).  -> (rank, world, torch device or None)"""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return 0, 1, None
    import torch
    import torch.distributed as dist
    rank, local = int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("FD_BENCH_BACKEND", "nccl")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29500")
    if backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    a.device = local
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, world, torch.device("cuda", local)


LAST_TIMINGS = {}      # stage times of the last `index` run in this process (bench.py's drop-in leg reads them)


def _shard_prefix(prefix, rank, world):
    return f"{prefix}.shard{rank}of{world}"


def cmd_index(a):
    import folddisco_amd as fd
    from folddisco_amd import indexio, structure
    if getattr(a, "coords", False) and int(os.environ.get("WORLD_SIZE", "1")) > 1:      # before any rank opens a device or parses a file
        print("[FAIL] index --coords writes the coordinate store from one rank only: build the index as it is and run `coords -i PREFIX` afterwards")
        sys.exit(1)
    rank, world, _dev = _init_dist(a)
    # an input that is a file is a Foldcomp database (build_index.rs:109-123): structures = its entries in key order, names from
    # DB.lookup, ids for the reader = database keys
    a.fc = structure.FoldcompDb(a.pdbs) if structure.is_foldcomp_db(a.pdbs) else None
    if a.fc is not None:
        keep = [k for k, nm in enumerate(a.fc.names) if nm]
        all_paths, a.fc_keys = [a.fc.names[k] for k in keep], a.fc.keys[keep]
    else:
        all_paths, a.fc_keys = _load_paths(a.pdbs, a.recursive), None
    if not all_paths:
        sys.exit(f"[FAIL] no structures under {a.pdbs}")
    prefix = a.index or (_default_index_prefix(a.pdbs))
    if world > 1:
        return _cmd_index_sharded(a, fd, indexio, structure, all_paths, prefix, rank, world)
    paths = all_paths
    import time
    T = a.timings = {"ingest_s": 0.0, "gpu_build_s": 0.0, "merge_s": 0.0, "export_write_s": 0.0, "chunks": 0}
    t_all = time.perf_counter()
    ctx = fd.Context(a.device)
    # The reference walks its input in chunks and parses / hashes a chunk in parallel (controller/mod.rs:282-348).  Here a host thread
    # ingests chunk k + 1 (native, multi-threaded: csrc/fd_ingest.cpp; a structure above the reference's hard-wired 65,535 residues keeps its id but has no hashes,
    # nres 0 and plddt 0, controller/mod.rs:313-318) WHILE the GPU builds the sub-index of chunk k (one fdgpu_index_build call, < 2^32 residue
    # pairs); the sub-indices stay resident in HBM and are concatenated per hash on the device (fdgpu_index_merge, in rounds of 64), so
    # the index crosses the bus once, in the reference's on-disk layout.
    from concurrent.futures import ThreadPoolExecutor
    tid_pool = ThreadPoolExecutor(1)
    tids_f = tid_pool.submit(lambda: [indexio.parse_path_by_id_type(x, a.id) for x in paths])      # 20 ms of Python per 20,000 paths: under the ingest
    cw = None
    if getattr(a, "coords", False):               # --coords: every parsed chunk goes to the store's section files as well (no second ingest)
        cw = indexio.CoordWriter(prefix + ".coords")
        a.coord_sink = cw.add
    try:
        parts, nres, plddt = _build_chunks(a, fd, structure, ctx, paths, 0, resident=True)
    except BaseException:
        if cw is not None:
            cw.abort()
        raise
    t0 = time.perf_counter()
    ix = _merge_resident(fd, parts)
    ctx.synchronize()
    T["merge_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ix.save(prefix)                               # the library writes PREFIX and PREFIX.offset itself (byte-identical to save_offset_to_file)
    T["save_s"] = time.perf_counter() - t0
    n_hashes, value_len = ix.num_hashes, ix.value_len
    indexio.save_lookup(prefix + ".lookup", tids_f.result(), nres, plddt, db_keys=a.fc_keys)
    tid_pool.shutdown()
    indexio.save_type(prefix + ".type", len(paths), grid_width=a.grid, max_residue=a.max_residue, nbin_angle=a.angle, nbin_dist=a.distance, hash_type=HASH_TYPE_NAMES[a.hash_type], multiple_bins=a.multi,
                      **(dict(input_format="FCZDB", foldcomp_db=a.pdbs) if a.fc is not None else {}))
    T["export_write_s"] = time.perf_counter() - t0
    if cw is not None:
        t0 = time.perf_counter()
        cw.close(indexio.index_stamp(prefix))
        T["coords_s"] = time.perf_counter() - t0
    T["total_s"] = time.perf_counter() - t_all
    T["structures"] = len(paths)
    LAST_TIMINGS.clear()
    LAST_TIMINGS.update(T)
    if a.verbose:
        print(f"[DONE] {len(paths)} structures, {n_hashes} hashes, {value_len} value bytes -> {prefix}", file=sys.stderr)
        print("[TIME] total %.2f s = %.0f structures/s; ingest %.2f s (host threads, overlapped with the GPU), GPU builds %.2f s, device merge %.2f s, "
              "export + files %.2f s" % (T["total_s"], len(paths) / max(T["total_s"], 1e-9), T["ingest_s"], T["gpu_build_s"], T["merge_s"], T["export_write_s"]), file=sys.stderr)


def _merge_resident(fd, parts):
    """sub-indices resident in HBM -> one resident index (fdgpu_index_merge takes at most 64 parts: merge in rounds)"""
    g = max(2, min(64, int(os.environ.get("FD_MERGE_GROUP", "64"))))      # parts per fdgpu_index_merge call (tests lower it to exercise the rounds)
    while len(parts) > 1:
        nxt = []
        for k in range(0, len(parts), g):
            grp = parts[k:k + g]
            nxt.append(fd.FolddiscoIndexSet(grp).merge() if len(grp) > 1 else grp[0])
        parts = nxt
    return parts[0]


def _default_index_prefix(pdbs: str) -> str:
    """build_index.rs:75-88 / controller/io.rs:460-470: DIR_folddisco; a database named X_foldcomp gives X_folddisco"""
    p = pdbs.rstrip("/")
    return p.replace("_foldcomp", "_folddisco") if p.endswith("_foldcomp") else p + "_folddisco"


# The reference's skip threshold is NOT its -n flag: Folddisco::new hard-wires max_residue = DEFAULT_MAX_RESIDUE = 65535
# (controller/mod.rs:40,124), set_max_residue (mod.rs:189) has no caller, and the test at mod.rs:313 therefore compares with 65535 whatever
# -n says; -n/--residue (cli/main.rs:42, default 50000) only lands in PREFIX.type (build_index.rs:222).  A structure of 50,001 ... 65,535
# residues is indexed by the reference, so it is indexed here.
REF_SKIP_MAX_RESIDUE = 65535


def _ingest(a, structure, chunk, pos0):
    """native ingest of one chunk of the input (files, or entries pos0 ... of the Foldcomp database) + the reference's warnings"""
    sink = getattr(a, "coord_sink", None)      # the coordinate store's writer, when one is being written (index --coords, update, coords)
    if a.fc is not None:
        ps, nres_c, plddt_c, raw, ok, *lab = structure.read_packed(a.fc_keys[pos0:pos0 + len(chunk)], threads=a.threads, max_residue=REF_SKIP_MAX_RESIDUE, foldcomp=a.fc,
                                                                   labels=sink is not None)
    else:
        ps, nres_c, plddt_c, raw, ok, *lab = structure.read_packed(chunk, threads=a.threads, max_residue=REF_SKIP_MAX_RESIDUE, labels=sink is not None)
    if sink is not None:
        from folddisco_amd import indexio
        sink(indexio.CoordArrays(ps, lab[0]["chain"], lab[0]["resname_std"], lab[0]["serial"]))
    for k in np.nonzero(ok == 0)[0]:
        print(f"[WARN] {chunk[k]} could not be read. Skipping", file=sys.stderr)
    for k in np.nonzero(raw > REF_SKIP_MAX_RESIDUE)[0]:
        print(f"[WARN] {chunk[k]} has too many residues. Skipping", file=sys.stderr)
    return ps, nres_c, plddt_c, raw, ok


def _build_chunks(a, fd, structure, ctx, paths, first_id, resident=False):
    """chunked GPU builds of paths (ids first_id ...), double-buffered: a host thread ingests chunk k + 1 while the GPU builds chunk k
    -> (sub-indices: resident FolddiscoIndex objects, or exported (value, hashes, offsets) triples; nres; plddt)"""
    import time
    from concurrent.futures import ThreadPoolExecutor
    T = getattr(a, "timings", None) or {}
    nres_all, plddt_all, parts = [], [], []
    starts = list(range(0, len(paths), a.chunk))

    def ingest(c0):
        t0 = time.perf_counter()
        r = _ingest(a, structure, paths[c0:c0 + a.chunk], first_id + c0)      # native, multi-threaded; releases the GIL
        return r, time.perf_counter() - t0
    with ThreadPoolExecutor(1) as pool:
        fut = pool.submit(ingest, starts[0]) if starts else None
        if resident:
            ctx.L.fdgpu_reserve_staging(ctx.h)      # the save's page-locked staging slots, made while the first chunk is parsed (this thread only waits otherwise)
        for k, c0 in enumerate(starts):
            (ps, nres_c, plddt_c, raw, ok), t_ing = fut.result()
            fut = pool.submit(ingest, starts[k + 1]) if k + 1 < len(starts) else None      # the next chunk is parsed while this one is built
            T["ingest_s"] = T.get("ingest_s", 0.0) + t_ing
            nres_all.append(nres_c)
            plddt_all.append(np.where(nres_c > 0, plddt_c, np.float32(0.0)).astype(np.float32))
            t0 = time.perf_counter()
            batch = ctx.upload(ps)
            ix = fd.FolddiscoIndex.build(ctx, batch, first_id=first_id + c0, nbin_dist=a.distance, nbin_angle=a.angle, dist_cutoff=a.grid, hash_type=a.hash_type, multiple_bins=a.multi)
            if resident:
                parts.append(ix)
            else:
                parts.append(ix.export())
                del ix
            del batch
            ctx.synchronize()
            T["gpu_build_s"] = T.get("gpu_build_s", 0.0) + time.perf_counter() - t0
            T["chunks"] = T.get("chunks", 0) + 1
    z = lambda dt: np.zeros(0, dt)
    if not parts and resident:
        parts = [fd.FolddiscoIndex.build(ctx, ctx.upload(fd.PackedStructures.concat([])), first_id=first_id)]
    return parts, (np.concatenate(nres_all) if nres_all else z(np.uint64)), (np.concatenate(plddt_all) if plddt_all else z(np.float32))


def _cmd_index_sharded(a, fd, indexio, structure, paths, prefix, rank, world):
    """Index build sharded by structure: rank r indexes the contiguous id range shard_range(r), no data-path collective;
    the shards stay on disk (PREFIX.shard<r>of<W>, used by the sharded query) and rank 0 concatenates them per hash into the
    reference's single PREFIX / PREFIX.offset."""
    import torch.distributed as dist
    from folddisco_amd import dist as fdist
    lo, hi = fdist.shard_range(rank, world, len(paths))
    ctx = fd.Context(a.device)
    a.timings = {}
    parts, nres, plddt = _build_chunks(a, fd, structure, ctx, paths[lo:hi], lo, resident=True)
    local = _merge_resident(fd, parts)              # the rank's chunks merged on the device
    local.save(_shard_prefix(prefix, rank, world))  # the shard stays on disk for the sharded query
    # ONE index for the database without the host (Option A; csrc/fd_shard_index.hip): hash ranges of equal posting bytes, piece j of
    # every rank's sub-index to rank j — ncclSend / ncclRecv inside the library when the ranks have a GPU each (backend nccl), torch.distributed objects
    # under gloo —, per-hash concatenation of the pieces on the device, every rank writes its regions of PREFIX / PREFIX.offset
    # (FD_INDEX_EXCHANGE=objects keeps the transport-free form reachable under nccl as well: a fall-back should the N-rank ncclSend / ncclRecv group —
    # executed so far with a world of one only — misbehave on a node)
    if dist.get_backend() == "nccl" and os.environ.get("FD_INDEX_EXCHANGE", "rccl") != "objects":
        comm = fdist.Comm(ctx, rank, world)
        rng, hb, vb, ht, vt = comm.single_index(local)
    else:
        comm = None
        rng, hb, vb, ht, vt = fdist.single_index_over_process_group(ctx, local)
    if rank == 0:
        for ext in ("", ".offset"):                 # regions are written in place: a stale file of another size must not survive beside them
            if os.path.exists(prefix + ext):
                os.remove(prefix + ext)
    dist.barrier()
    rng.save_part(prefix, hb, vb, ht, vt, write_header=(rank == 0), is_last=(rank == world - 1))
    del rng, comm
    box = [None] * world
    dist.all_gather_object(box, (nres, plddt))
    dist.barrier()
    if rank == 0:
        indexio.save_lookup(prefix + ".lookup", [indexio.parse_path_by_id_type(x, a.id) for x in paths], np.concatenate([b[0] for b in box]), np.concatenate([b[1] for b in box]), db_keys=a.fc_keys)
        indexio.save_type(prefix + ".type", len(paths), grid_width=a.grid, max_residue=a.max_residue, nbin_angle=a.angle, nbin_dist=a.distance, hash_type=HASH_TYPE_NAMES[a.hash_type], multiple_bins=a.multi,
                          **(dict(input_format="FCZDB", foldcomp_db=a.pdbs) if a.fc is not None else {}))
        if a.verbose:
            print(f"[DONE] {len(paths)} structures over {world} ranks, {ht} hashes, {vt} value bytes -> {prefix}", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


INDEX_FILES = ("", ".offset", ".lookup", ".type")


def _open_store(path, prefix, n_structures=None):
    """PREFIX.coords for a command that is about to use it: a store the reader refuses (indexio.CoordStore.open: inconsistent, or its stamp disagrees
    with the index files at `prefix`; prefix None skips the stamp) ends the command with status 1, an unreadable one with status 2"""
    from folddisco_amd import indexio
    try:
        st = indexio.CoordStore.open(path, check_prefix=prefix)
        if n_structures is not None and st.n_struct != n_structures:
            raise indexio.CoordStoreError(f"{path} holds {st.n_struct} structures, the index {n_structures}")
    except indexio.CoordStoreError as e:
        print(f"[FAIL] coordinate store refused: {e}")
        sys.exit(1)
    except OSError as e:
        print(f"[FAIL] {path}: unreadable ({e})", file=sys.stderr)
        sys.exit(2)
    return st


def _tmp_stamp(tmp, n_rows):
    """the stamp a store gets that is written beside index files still under their temporary names (they are renamed, not rewritten)"""
    return n_rows, os.path.getsize(tmp), os.path.getsize(tmp + ".offset")


def _update_plan(a):
    """everything `update` decides before it touches a device: the index's rows and settings, the keep mask, the files to append.
    Refusals exit with status 1 and change nothing."""
    from folddisco_amd import indexio
    if not a.index:
        sys.exit("[FAIL] -i/--index is required")
    if not a.pdbs and not a.remove:
        sys.exit("[FAIL] update: give structures to append (-p) and / or a file of tids to remove (--remove)")
    for ext in INDEX_FILES:
        if not os.path.exists(a.index + ext):
            sys.exit(f"[FAIL] {a.index}{ext} not found")
    rows = indexio.read_lookup_rows(a.index + ".lookup")
    tids = [r.rstrip("\n").split("\t")[1] for r in rows]
    cfg = indexio.load_type(a.index + ".type")
    with open(a.index + ".type") as f:
        type_text = f.read()
    fczdb = cfg.get("input_format") == "FCZDB"
    keep = np.ones(len(rows), dtype=bool)
    if a.remove:
        with open(a.remove) as f:
            gone = [line.strip() for line in f if line.strip()]
        known = set(tids)
        unknown = [t for t in dict.fromkeys(gone) if t not in known]
        if unknown:
            sys.exit(f"[FAIL] update: {len(unknown)} tid(s) of {a.remove} are not in {a.index}.lookup: " + ", ".join(unknown[:10]) +
                     (" ..." if len(unknown) > 10 else ""))
        gone = set(gone)
        keep = np.array([t not in gone for t in tids], dtype=bool)
        if not keep.any():
            sys.exit("[FAIL] update: removing every structure is refused (build a new index with `index`)")
    add_paths = []
    if a.pdbs:
        if fczdb:
            sys.exit("[FAIL] update: appending to an index built from a Foldcomp database is not supported (-p); --remove is")
        add_paths = _load_paths(a.pdbs, a.recursive)
        if not add_paths:
            sys.exit(f"[FAIL] no structures under {a.pdbs}")
    store = _open_store(a.index + ".coords", a.index, len(rows)) if os.path.isfile(a.index + ".coords") else None      # a stale store is refused here
    return dict(rows=rows, keep=keep, cfg=cfg, type_text=type_text, fczdb=fczdb, add_paths=add_paths, store=store)


def cmd_update(a):
    """`update`: remove structures from an index and / or append new ones without a rebuild.  The result is byte for byte the index `index`
    builds over (kept structures in their old order) + (added structures in walk order): the resident index is pruned on the device
    (fdgpu_index_remove), the added structures are built at the next ids with the hash parameters of PREFIX.type and merged on the device
    (fdgpu_index_merge).  The four files are written under temporary names beside the output prefix and then renamed over it."""
    plan = _update_plan(a)
    if a.verify:
        _verify_files(a.index)
    import folddisco_amd as fd
    from folddisco_amd import indexio, structure
    cfg, keep, add_paths = plan["cfg"], plan["keep"], plan["add_paths"]
    # hash parameters of the existing index, never the command line's defaults
    hp = _type_hash_params(cfg)
    a.distance, a.angle, a.grid, a.hash_type, a.multi = hp["nbin_dist"], hp["nbin_angle"], hp["dist_cutoff"], hp["hash_type"], cfg.get("multiple_bin")
    a.fc = None
    n_kept = int(keep.sum())
    ctx = fd.Context(a.device)
    v, h, o = indexio.read_index_files(a.index)
    ix = fd.FolddiscoIndex.load(ctx, h, o, v, len(keep))
    del v, h, o
    if a.verify:                                 # before the prune or the merge uses its offsets and ids as addresses
        _stop_if_unsound(ix.verify(), a.index)
    if n_kept < len(keep):
        pruned = ix.remove(keep)
        del ix                                   # the loaded index is released once the pruned one exists
        ix = pruned
    rows = indexio.update_lookup_rows(plan["rows"], keep, keep_db_keys=plan["fczdb"])
    out = a.output or a.index
    tmp = f"{out}.update-tmp{os.getpid()}"
    cw = None
    if plan["store"] is not None:                # the store follows the index: the kept slices now, the added structures' arrays as they are parsed
        cw = indexio.CoordWriter(tmp + ".coords")
        try:
            cw.add((plan["store"], None if n_kept == len(keep) else np.nonzero(keep)[0]))
        except BaseException:
            cw.abort()
            raise
        a.coord_sink = cw.add
    try:
        _update_rest(a, fd, indexio, structure, ctx, plan, ix, rows, add_paths, n_kept, keep, out, tmp, cw)
    except BaseException:
        if cw is not None:
            cw.abort()
        raise


def _update_rest(a, fd, indexio, structure, ctx, plan, ix, rows, add_paths, n_kept, keep, out, tmp, cw):
    if add_paths:
        a.timings = {}
        parts, nres, plddt = _build_chunks(a, fd, structure, ctx, add_paths, n_kept, resident=True)
        ix = _merge_resident(fd, [ix] + parts)
        del parts
        rows += indexio.lookup_rows(n_kept, [indexio.parse_path_by_id_type(x, a.id) for x in add_paths], nres, plddt)
    if a.verify:                                 # the result, before anything is written
        _stop_if_unsound(ix.verify(), "the updated index; nothing was written")
    exts = INDEX_FILES + ((".coords",) if cw is not None else ())
    try:
        ix.save(tmp)
        with open(tmp + ".lookup", "w", newline="") as f:
            f.writelines(rows)
        with open(tmp + ".type", "w") as f:
            f.write(indexio.update_type_text(plan["type_text"], len(rows)))
        if cw is not None:
            cw.close(_tmp_stamp(tmp, len(rows)))
        for ext in exts:
            os.replace(tmp + ext, out + ext)
    finally:
        for ext in exts:
            if os.path.exists(tmp + ext):
                os.remove(tmp + ext)
    if a.verbose:
        print(f"[DONE] {len(keep) - n_kept} removed, {len(add_paths)} added: {len(rows)} structures, {ix.num_hashes} hashes, {ix.value_len} value bytes -> {out}",
              file=sys.stderr)


def _verify_files(prefix):
    """the file checks of `verify` (indexio.check_index_files) -> the index's arrays and its number of structures; exits with status 2 when a file is
    missing or unreadable, with status 1 and a [FAIL] line when the files contradict each other"""
    from folddisco_amd import indexio
    for ext in INDEX_FILES:
        if not os.path.isfile(prefix + ext):
            print(f"[FAIL] {prefix}{ext} not found", file=sys.stderr)
            sys.exit(2)
    try:
        bad = indexio.check_index_files(prefix)
        if not bad:
            v, h, o = indexio.read_index_files(prefix)
            with open(prefix + ".lookup") as f:
                n = sum(1 for _ in f)
    except (OSError, ValueError, UnicodeDecodeError) as e:
        print(f"[FAIL] {prefix}: unreadable ({e})", file=sys.stderr)
        sys.exit(2)
    if bad:
        print("[FAIL] index files are inconsistent: " + "; ".join(bad))
        sys.exit(1)
    return v, h, o, n


def _stop_if_unsound(report, what):
    """--verify of query / update: an unsound index ends the command with the verify message and status 1"""
    if not report.ok:
        print(f"{report} ({what})")
        sys.exit(1)


def _type_hash_params(cfg) -> dict:
    """the hash parameters PREFIX.type records, as the keywords of FolddiscoIndex.build / get_geometric_hash_as_u32 (multiple_bins apart)"""
    return dict(nbin_dist=int(cfg.get("num_bin_dist", 0)), nbin_angle=int(cfg.get("num_bin_angle", 0)), dist_cutoff=float(cfg.get("grid_width", 20.0)),
                hash_type=hash_type_index(cfg.get("hash_type", "PDBTrRosetta")))


def _windows(ids, width, n):
    """windows [lo, hi) of at most `width` structures that cover the ascending unique ids: -> (lo, hi, first, end) with ids[first:end] inside"""
    k = 0
    while k < len(ids):
        lo = int(ids[k])
        hi = min(lo + width, n)
        end = int(np.searchsorted(ids, hi))
        yield lo, hi, k, end
        k = end


def _structures_check(a, ctx, ix, store, cfg, n, tids):
    """`verify --structures`: does the index describe these coordinates?  Per window of structures: the index's rows (fdgpu_index_rows) against
    the hashes of the store's slice (fdgpu_hash_batch with the parameters of PREFIX.type).  -> (structures, hashes) compared; the first
    structure that differs ends the command with status 1"""
    import folddisco_amd as fd
    hp = _type_hash_params(cfg)
    raw = hp["hash_type"] in (2, 4, 5, 6)            # encodings the hasher serves in the raw order only: sorted and made unique here
    total = 0
    for lo, hi, _, _ in _windows(np.arange(n), a.window, n):
        got_h, got_off = ix.rows(lo, hi)
        batch = ctx.upload(store.slice(lo, hi).ps)
        want_h, want_off = fd.get_geometric_hash_as_u32(ctx, batch, sort_dedup=not raw, **hp)
        del batch
        if raw:
            owner = np.repeat(np.arange(hi - lo, dtype=np.uint64), np.diff(want_off.astype(np.int64)))
            key = np.unique(owner << np.uint64(32) | want_h.astype(np.uint64))
            want_h = (key & np.uint64(0xffffffff)).astype(np.uint32)
            want_off = np.searchsorted(key >> np.uint64(32), np.arange(hi - lo + 1, dtype=np.uint64)).astype(np.uint64)
        total += len(got_h)
        if np.array_equal(got_off, want_off) and np.array_equal(got_h, want_h):
            continue
        for s in range(hi - lo):
            g, w = got_h[int(got_off[s]):int(got_off[s + 1])], want_h[int(want_off[s]):int(want_off[s + 1])]
            if not np.array_equal(g, w):
                only_ix, only_co = np.setdiff1d(g, w), np.setdiff1d(w, g)
                show = lambda x: str(int(x[0])) if len(x) else "none"
                print(f"[FAIL] structure {lo + s} {tids[lo + s]}: index row {len(g)} hashes, coordinates {len(w)}, first hash only in the index / "
                      f"only in the coordinates: {show(only_ix)} / {show(only_co)}")
                sys.exit(1)
    return n, total


def cmd_verify(a):
    """`verify`: is the index at PREFIX well formed?  File checks (sizes, .lookup ids, chunk_size), then every posting list decoded once, on the
    device (fdgpu_index_verify) or with --host on the CPU (fdgpu_verify_host; no device is opened).  With --structures, behind those: does the
    index describe the coordinates of its store (_structures_check)?  Exit status 0 / 1, 2 for unreadable input."""
    from folddisco_amd import indexio
    v, h, o, n = _verify_files(a.index)
    if os.path.isfile(a.index + ".coords"):      # part of the file checks: header, sections, res_off, stamp
        st = _open_store(a.index + ".coords", a.index, n)
        print(f"[OK] {a.index}.coords: {st.n_struct} structures, {st.n_res} residues, stamp matches the index files")
    if a.structures:                             # its refusals come before any device is opened
        if a.host:
            sys.exit("[FAIL] verify --structures: there is no host hasher in the library; run it without --host")
        if a.window < 1:
            sys.exit("[FAIL] verify --structures: --window must be at least 1")
        cfg = indexio.load_type(a.index + ".type")
        if cfg.get("multiple_bin"):
            sys.exit("[FAIL] verify --structures: the index was built with --multiple-bins, which the batch hasher does not serve")
        cpath = a.coords or a.index + ".coords"
        if not os.path.isfile(cpath):
            sys.exit(f"[FAIL] verify --structures: {cpath} not found; run `coords -i {a.index}` first" if not a.coords else
                     f"[FAIL] verify --structures: {cpath} not found")
        if a.coords:
            st = _open_store(cpath, a.index, n)
        tids = [r.rstrip("\n").split("\t")[1] for r in indexio.read_lookup_rows(a.index + ".lookup")]
    if a.host:
        rep = indexio.verify_host(v, h, o, n, threads=a.threads)
    else:
        import folddisco_amd as fd
        ctx = fd.Context(a.device)
        ix = fd.FolddiscoIndex.load(ctx, h, o, v, n)
        rep = ix.verify()
    print(rep)
    if a.verbose:
        print(f"[INFO] {a.index}: {len(h)} hashes, {len(v)} value bytes, {n} structures; checked on the {'host' if a.host else 'device'}"
              + ("" if rep.list_stage else "; the offsets table is damaged, the lists were not decoded"), file=sys.stderr)
    if a.structures and rep.ok:
        ns, nh = _structures_check(a, ctx, ix, st, cfg, n, tids)
        print(f"[OK] {a.index}: the index describes the coordinates of {cpath}: {ns} structures, {nh} hashes compared")
    sys.exit(0 if rep.ok else 1)


def _ids_of_tids(cmd, asked, path, tids, index):
    """the ids of the tids asked for, in their order, every row that carries the tid; status 1 and a [FAIL] line for a tid the index does not hold"""
    where = {}
    for k, t in enumerate(tids):
        where.setdefault(t, []).append(k)
    unknown = [t for t in dict.fromkeys(asked) if t not in where]
    if unknown:
        print(f"[FAIL] {cmd}: {len(unknown)} tid(s) of {path} are not in {index}.lookup: " + ", ".join(unknown[:10]) + (" ..." if len(unknown) > 10 else ""))
        sys.exit(1)
    return np.array([k for t in asked for k in where[t]], dtype=np.int64)


def _rows_plan(a):
    """everything `rows` decides before it opens a device: -> (structures of the index, chosen ids in the order asked for, their tids).  Status 2
    for missing or unreadable files, status 1 and a [FAIL] line for a refusal; nothing is written in either case."""
    from folddisco_amd import indexio
    if a.range is not None and a.tids is not None:
        sys.exit("[FAIL] rows: give at most one of --range LO:HI and --tids FILE")
    if a.window < 1:
        sys.exit("[FAIL] rows: --window must be at least 1")
    for f in [a.index + ext for ext in INDEX_FILES] + ([a.tids] if a.tids is not None else []):
        if not os.path.isfile(f):
            print(f"[FAIL] {f} not found", file=sys.stderr)
            sys.exit(2)
    try:
        bad = indexio.check_index_files(a.index)
        tids = [r.rstrip("\n").split("\t")[1] for r in indexio.read_lookup_rows(a.index + ".lookup")]
        asked = None
        if a.tids is not None:
            with open(a.tids) as f:
                asked = [line.strip() for line in f if line.strip()]
    except (OSError, ValueError, UnicodeDecodeError) as e:
        print(f"[FAIL] rows: unreadable input ({e})", file=sys.stderr)
        sys.exit(2)
    if bad:
        print("[FAIL] index files are inconsistent: " + "; ".join(bad))
        sys.exit(1)
    n = len(tids)
    if asked is not None:
        ids = _ids_of_tids("rows", asked, a.tids, tids, a.index)
    else:
        lo, hi = 0, n
        if a.range is not None:
            try:
                lo_s, hi_s = a.range.split(":")
                lo, hi = int(lo_s) if lo_s else 0, int(hi_s) if hi_s else n
            except ValueError:
                sys.exit(f"[FAIL] rows: --range {a.range}: LO:HI expected")
            if not 0 <= lo <= hi <= n:
                print(f"[FAIL] rows: --range {a.range} is not inside the index's {n} structures")
                sys.exit(1)
        ids = np.arange(lo, hi, dtype=np.int64)
    return n, ids, tids


def cmd_rows(a):
    """`rows`: the hashes of chosen structures read back from the index at PREFIX (the transposed index), as OUT.npz with hashes, row_off, ids and
    tids: hashes[row_off[k]: row_off[k + 1]] are the ascending hashes whose posting lists hold structure ids[k].  The index is walked in windows
    of --window structures that cover the chosen ids, on the device (fdgpu_index_rows) or with --host on the CPU (fdgpu_rows_host; no device is
    opened); rows that were not asked for are dropped on the host.  No structure file is read."""
    from folddisco_amd import indexio
    n, ids, tids = _rows_plan(a)
    if not a.output:
        sys.exit("[FAIL] rows: -o OUT.npz is required")
    try:
        v, h, o = indexio.read_index_files(a.index)
        if a.host:
            if a.verify:
                _stop_if_unsound(indexio.verify_host(v, h, o, n, threads=a.threads), a.index)
            window = lambda lo, hi: indexio.rows_host(v, h, o, n, lo=lo, hi=hi, threads=a.threads)
        else:
            import folddisco_amd as fd
            ctx = fd.Context(a.device)
            ix = fd.FolddiscoIndex.load(ctx, h, o, v, n)
            del v, h, o
            if a.verify:                             # before the walk uses its offsets as addresses
                _stop_if_unsound(ix.verify(), a.index)
            window = ix.rows
        uniq = np.unique(ids)
        piece = [None] * len(uniq)                   # the row of every chosen structure
        n_windows = 0
        for lo, hi, k0, k1 in _windows(uniq, a.window, n):
            wh, woff = window(lo, hi)
            n_windows += 1
            for k in range(k0, k1):
                s = int(uniq[k]) - lo
                piece[k] = wh[int(woff[s]):int(woff[s + 1])]
        at = np.searchsorted(uniq, ids)
        lens = np.array([len(piece[k]) for k in at], dtype=np.uint64)
        row_off = np.zeros(len(ids) + 1, np.uint64)
        row_off[1:] = np.cumsum(lens, dtype=np.uint64)
        hashes = np.concatenate([piece[k] for k in at]).astype(np.uint32, copy=False) if len(ids) else np.zeros(0, np.uint32)
    except (OSError, ValueError) as e:
        print(f"[FAIL] rows: {e}", file=sys.stderr)
        sys.exit(2 if isinstance(e, OSError) else 1)
    tmp = f"{a.output}.rows-tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            np.savez(f, hashes=hashes, row_off=row_off, ids=ids.astype(np.uint64), tids=np.array([tids[k] for k in ids], dtype=str))
        os.replace(tmp, a.output)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    print(f"[OK] {a.output}: {len(ids)} structures, {len(hashes)} hashes, longest row {int(lens.max()) if len(ids) else 0}")
    if a.verbose:
        print(f"[INFO] rows of {a.index} on the {'host' if a.host else 'device'}: {n_windows} window(s) of up to {a.window} structures", file=sys.stderr)


def _dups_plan(a, cmd="dups"):
    """everything `dups` (and `overlap`, which plans like it) decides before it opens a device: -> (prefixes, their tids).  Status 2 for missing
    or unreadable files, status 1 and a [FAIL] line for a refusal; nothing is written in either case."""
    if a.max_pairs < 0:
        sys.exit(f"[FAIL] {cmd}: --max-pairs must not be negative")
    _min_jaccard_plan(a, cmd)
    return _sig_plan(a, cmd)


def _min_jaccard_plan(a, cmd):
    """--min-jaccard F: outside (0, 1] (NaN too) is a refusal; given, it implies --confirm"""
    if getattr(a, "min_jaccard", None) is None:
        return
    if not 0.0 < a.min_jaccard <= 1.0:
        sys.exit(f"[FAIL] {cmd}: --min-jaccard {a.min_jaccard} is outside (0, 1]")
    a.confirm = True


def _sig_plan(a, cmd):
    """what `dups` and `neighbors` check alike before a device is opened: the threshold and the window, that -i (and --against) name single,
    consistent indices that are not the same one and whose .type files agree -> (prefixes, their tids)"""
    import glob
    from folddisco_amd import indexio
    if not 0.0 < a.min_similarity <= 1.0:            # NaN fails it too
        sys.exit(f"[FAIL] {cmd}: --min-similarity {a.min_similarity} is outside (0, 1]")
    if a.window < 1:
        sys.exit(f"[FAIL] {cmd}: --window must be at least 1")
    prefixes = [a.index] + ([a.against] if a.against is not None else [])
    if len(prefixes) == 2 and os.path.abspath(prefixes[0]) == os.path.abspath(prefixes[1]):
        sys.exit(f"[FAIL] {cmd}: --against {a.against} is the index itself; leave it out to look for duplicates inside one index")
    for p in prefixes:
        if not os.path.isfile(p) and glob.glob(glob.escape(p) + ".shard*of*"):
            print(f"[FAIL] {cmd}: {p} is a sharded index; write the single index first (`reshard -i {p} --from V --to 1`)")
            sys.exit(1)
        for ext in INDEX_FILES:
            if not os.path.isfile(p + ext):
                print(f"[FAIL] {p}{ext} not found", file=sys.stderr)
                sys.exit(2)
    try:
        bad = [b for p in prefixes for b in indexio.check_index_files(p)]
        tids = [[r.rstrip("\n").split("\t")[1] for r in indexio.read_lookup_rows(p + ".lookup")] for p in prefixes]
        texts = []
        for p in prefixes:
            with open(p + ".type") as f:
                texts.append(f.read())
    except (OSError, ValueError, UnicodeDecodeError) as e:
        print(f"[FAIL] {cmd}: unreadable input ({e})", file=sys.stderr)
        sys.exit(2)
    if bad:
        print("[FAIL] index files are inconsistent: " + "; ".join(bad))
        sys.exit(1)
    key = indexio.check_joinable(texts)
    if key is not None:
        print(f"[FAIL] {cmd}: the two indices' .type files differ in {key}: signatures of indices built with different settings are not comparable")
        sys.exit(1)
    return prefixes, tids


def _dups_signatures(a, ctx, prefix, n):
    """the signature table of one index: loaded, checked if --verify, reduced, released"""
    from folddisco_amd import indexio
    v, h, o = indexio.read_index_files(prefix)
    if a.host:
        if a.verify:
            _stop_if_unsound(indexio.verify_host(v, h, o, n, threads=a.threads), prefix)
        return np.array(indexio.signatures_host(v, h, o, n, threads=a.threads))
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.load(ctx, h, o, v, n)
    del v, h, o
    if a.verify:
        _stop_if_unsound(ix.verify(), prefix)
    return np.array(ix.signatures(window=a.window))


def _dups_overlaps(a, ctx, prefixes, tids, ia, ib, stats=None, verify=False):
    """the exact row overlaps of the pairs (ia[k] of the first index, ib[k] of the second one, or of the first if there is one only) ->
    (inter, n_a, n_b) as int64 arrays, from the tiling drivers: indexio.row_overlaps on the device, row_overlaps_host with --host.  At most
    --pool-mb (default 4096) megabytes of rows are resident at a time"""
    from folddisco_amd import indexio
    ia, ib = np.asarray(ia).astype(np.int64), np.asarray(ib).astype(np.int64)
    stats = a.overlap_stats = {"extractions": 0, "distinct": 0, "tiles": 0} if stats is None else stats      # what -v prints
    if not len(ia) and not verify:
        return tuple(np.zeros(0, np.int64) for _ in range(3))
    pool = int(getattr(a, "pool_mb", 4096)) * (1 << 20) // 4
    files = [indexio.read_index_files(p) + (len(t),) for p, t in zip(prefixes, tids)]
    if a.host:
        if verify:
            for p, (v, h, o, n) in zip(prefixes, files):
                _stop_if_unsound(indexio.verify_host(v, h, o, n, threads=a.threads), p)
        got = indexio.row_overlaps_host(files[0], files[1] if len(files) == 2 else None, ia, ib, window=a.window, pool_hashes=pool, threads=a.threads,
                                        stats=stats)
    else:
        import folddisco_amd as fd
        ixs = [fd.FolddiscoIndex.load(ctx, h, o, v, n) for v, h, o, n in files]
        del files
        if verify:
            for p, ix in zip(prefixes, ixs):
                _stop_if_unsound(ix.verify(), p)
        got = indexio.row_overlaps(ixs[0], ixs[1] if len(ixs) == 2 else None, ia, ib, window=a.window, pool_hashes=pool, stats=stats)
    return tuple(np.asarray(x).astype(np.int64) for x in got)


def _extractions(a):
    """the -v clause of the commands that confirm: a row may be extracted more than once when the pool is small"""
    st = getattr(a, "overlap_stats", None)
    return f" ({st['extractions']} row extractions for {st['distinct']} distinct rows)" if st else ""


def _jaccard_values(exact):
    """inter / max(union, 1) of every pair, from the integers"""
    return [int(i) / max(int(x) + int(y) - int(i), 1) for i, x, y in zip(*exact)]


def _dups_jaccard(a, ctx, prefixes, tids, ia, ib):
    """the exact Jaccard similarity of the pairs (ia[k] of the first index, ib[k] of the second one, or of the first if there is one only),
    from the rows of their structures"""
    return _jaccard_values(_dups_overlaps(a, ctx, prefixes, tids, ia, ib))


def _write_tsv(output, lines, cmd):
    """the lines to `output` under a temporary name, then renamed; to standard output without one"""
    if not output:
        sys.stdout.writelines(lines)
        return
    tmp = f"{output}.{cmd}-tmp{os.getpid()}"
    try:
        with open(tmp, "w") as f:
            f.writelines(lines)
        os.replace(tmp, output)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def cmd_dups(a):
    """`dups`: which structures are already there?  Every structure of the index at PREFIX is reduced to its signature (fdgpu_index_signatures:
    size, two digests and a 64-bucket MinHash sketch of its row) and the signatures are compared all against all, inside the index or, with
    --against, with those of a second one, on the device (fdgpu_signature_pairs) or with --host on the CPU (no device is opened).  One TSV row
    per reported pair, sorted by (id_a, id_b): id_a tid_a n_a id_b tid_b n_b match filled estimate class[ jaccard]; class is `identical` (same
    size and digests: the same hash set) or `similar` (estimate = match / filled of the sketches reaches --min-similarity); --confirm adds the
    exact Jaccard similarity from the rows of the reported structures (indexio.row_overlaps); --min-jaccard F implies it and keeps only the
    reported pairs whose exact similarity reaches F (indexio.jaccard_reaches).  It reports and removes nothing.  No structure file is read."""
    from folddisco_amd import indexio
    prefixes, tids = _dups_plan(a)
    two = len(prefixes) == 2
    thr64 = 64 if a.identical_only else indexio.signature_threshold(a.min_similarity)
    try:
        ctx = None
        if not a.host:
            import folddisco_amd as fd
            ctx = fd.Context(a.device)
        tabs = [_dups_signatures(a, ctx, p, len(t)) for p, t in zip(prefixes, tids)]
        A, B = tabs[0], (tabs[1] if two else None)
        try:
            pairs = indexio.signature_pairs_host(A, B, thr64=thr64, max_pairs=a.max_pairs, threads=a.threads) if a.host else \
                ctx.signature_pairs(A, B, thr64=thr64, max_pairs=a.max_pairs)
        except indexio.SignaturePairsOverflow as e:
            print(f"[FAIL] dups: {e.count} pairs reach the threshold {thr64}/64, more than --max-pairs {a.max_pairs}: raise --min-similarity or --max-pairs")
            sys.exit(1)
        if a.identical_only:
            pairs = pairs[(pairs["flags"] & indexio.SIG_IDENTICAL) != 0]
        jac = None
        if a.confirm:
            exact = _dups_overlaps(a, ctx, prefixes, tids, pairs["a"], pairs["b"])
            if a.min_jaccard is not None:            # only the reported pairs whose exact similarity reaches the floor
                keep = indexio.jaccard_reaches(exact[0], exact[1] + exact[2] - exact[0], a.min_jaccard)
                pairs, exact = pairs[keep], tuple(x[keep] for x in exact)
            jac = _jaccard_values(exact)
    except (OSError, ValueError) as e:
        print(f"[FAIL] dups: {e}", file=sys.stderr)
        sys.exit(2 if isinstance(e, OSError) else 1)
    tb = tids[1] if two else tids[0]
    lines = []
    for k, r in enumerate(pairs):
        ia, ib = int(r["a"]), int(r["b"])
        cols = [str(ia), tids[0][ia], str(int(A["n"][ia])), str(ib), tb[ib], str(int((B if two else A)["n"][ib])), str(int(r["match"])), str(int(r["filled"])),
                f"{float(r['estimate']):.4f}", "identical" if int(r["flags"]) & indexio.SIG_IDENTICAL else "similar"]
        if jac is not None:
            cols.append(f"{jac[k]:.4f}")
        lines.append("\t".join(cols) + "\n")
    _write_tsv(a.output, lines, "dups")
    n_ident = int(((pairs["flags"] & indexio.SIG_IDENTICAL) != 0).sum())
    print(f"[OK] {' x '.join(prefixes)}: {' x '.join(str(len(t)) for t in tids)} structures, {len(pairs)} pairs ({n_ident} identical), threshold {thr64}/64")
    if a.verbose:
        print(f"[INFO] dups on the {'host' if a.host else 'device'}: signatures of {sum(len(t) for t in tids)} structures ({sum(t.nbytes for t in tabs)} bytes)"
              + (f", {len(jac)} pairs confirmed from their rows" + _extractions(a) if jac is not None else ""), file=sys.stderr)


def _overlap_plan(a):
    """everything `overlap` decides before it opens a device: the planning of `dups`, then the pairs of --pairs FILE looked up in the .lookup
    files -> (prefixes, their tids, ids of the first index, ids of the second).  Status 2 for missing or unreadable files, status 1 and a
    [FAIL] line for a refusal; nothing is written in either case."""
    if a.pool_mb < 1:
        sys.exit("[FAIL] overlap: --pool-mb must be at least 1")
    if not os.path.isfile(a.pairs):
        print(f"[FAIL] {a.pairs} not found", file=sys.stderr)
        sys.exit(2)
    prefixes, tids = _dups_plan(a, "overlap")
    try:
        with open(a.pairs) as f:
            lines = [line.rstrip("\n") for line in f if line.strip()]
    except (OSError, UnicodeDecodeError) as e:
        print(f"[FAIL] overlap: unreadable input ({e})", file=sys.stderr)
        sys.exit(2)
    cols = [line.split("\t") for line in lines]
    bad = [k for k, c in enumerate(cols) if len(c) != 2 or not c[0] or not c[1]]
    if bad:
        print(f"[FAIL] overlap: {len(bad)} line(s) of {a.pairs} are not tid_a<TAB>tid_b, the first: {lines[bad[0]]!r}")
        sys.exit(1)
    out = []
    for side, (p, t) in enumerate(zip([prefixes[0], prefixes[-1]], [tids[0], tids[-1]])):
        where = {}
        for k, x in enumerate(t):
            where.setdefault(x, []).append(k)
        asked = list(dict.fromkeys(c[side] for c in cols))
        unknown = [x for x in asked if x not in where]
        if unknown:
            print(f"[FAIL] overlap: {len(unknown)} tid(s) of {a.pairs} are not in {p}.lookup: " + ", ".join(unknown[:10]) + (" ..." if len(unknown) > 10 else ""))
            sys.exit(1)
        twice = [x for x in asked if len(where[x]) > 1]
        if twice:
            print(f"[FAIL] overlap: {len(twice)} tid(s) of {a.pairs} name more than one row of {p}.lookup: " + ", ".join(twice[:10]) + (" ..." if len(twice) > 10 else ""))
            sys.exit(1)
        out.append(np.array([where[c[side]][0] for c in cols], dtype=np.int64))
    return prefixes, tids, out[0], out[1]


def cmd_overlap(a):
    """`overlap`: the exact similarity of given pairs of structures.  --pairs FILE holds one tid_a<TAB>tid_b per line (column 2 of PREFIX.lookup;
    with --against, tid_b is looked up in PREFIX2).  The rows of the named structures are kept on the device in sets of at most --pool-mb
    megabytes (fdgpu_index_rowset) and intersected pair by pair (fdgpu_rowset_intersect), or with --host on the CPU (no device is opened).  One
    TSV row per pair in the file's order: id_a tid_a n_a id_b tid_b n_b inter union jaccard, where inter = |R_a ∩ R_b| over the two rows,
    union = n_a + n_b - inter and jaccard = inter / max(union, 1); --min-jaccard F keeps the pairs that reach F (indexio.jaccard_reaches).
    Integers only: device and host write the same file.  No structure file is read."""
    prefixes, tids, ia, ib = _overlap_plan(a)
    from folddisco_amd import indexio
    stats = {"extractions": 0, "distinct": 0, "tiles": 0}
    try:
        ctx = None
        if not a.host:
            import folddisco_amd as fd
            ctx = fd.Context(a.device)
        inter, n_a, n_b = _dups_overlaps(a, ctx, prefixes, tids, ia, ib, stats=stats, verify=a.verify)
    except (OSError, ValueError) as e:
        print(f"[FAIL] overlap: {e}", file=sys.stderr)
        sys.exit(2 if isinstance(e, OSError) else 1)
    union = n_a + n_b - inter
    keep = indexio.jaccard_reaches(inter, union, a.min_jaccard) if a.min_jaccard is not None else np.ones(len(ia), bool)
    ta, tb = tids[0], tids[-1]
    lines = ["\t".join([str(int(ia[k])), ta[ia[k]], str(int(n_a[k])), str(int(ib[k])), tb[ib[k]], str(int(n_b[k])), str(int(inter[k])), str(int(union[k])),
                        f"{int(inter[k]) / max(int(union[k]), 1):.4f}"]) + "\n" for k in np.nonzero(keep)[0]]
    _write_tsv(a.output, lines, "overlap")
    print(f"[OK] {' x '.join(prefixes)}: {len(ia)} pairs, {stats['distinct']} distinct rows"
          + (f", {int(keep.sum())} at or above {a.min_jaccard}" if a.min_jaccard is not None else ""))
    if a.verbose:
        print(f"[INFO] overlap on the {'host' if a.host else 'device'}: {stats['extractions']} row extractions for {stats['distinct']} distinct rows, "
              f"{stats['tiles']} tile(s) within {a.pool_mb} MB", file=sys.stderr)


def cmd_neighbors(a):
    """`neighbors`: for every structure of the index at PREFIX its K nearest structures by signature, among the other structures of PREFIX or,
    with --against, among those of PREFIX2, selected on the device (fdgpu_signature_neighbors) or with --host on the CPU (no device is opened).
    --tids FILE restricts the queries to the structures with those tids; --min-similarity is the floor a neighbour must reach (default 1 / 64: one
    agreeing filled bucket).  One TSV row per neighbour, sorted by (id, rank): id tid n rank nb_id nb_tid nb_n match filled estimate
    class[ jaccard]; rank counts from 1, nearest first: by match / filled, then by filled, then by nb_id.  A structure without a neighbour gets
    no row.  This is the order of the sketches, not an exact nearest-neighbour search: --confirm adds the exact Jaccard similarity from the rows
    but does not reorder; --exact selects by the exact similarity instead (_neighbors_exact; --min-jaccard is its floor) and is refused together
    with --confirm or an explicit --min-similarity.  No structure file is read."""
    from folddisco_amd import indexio
    if a.min_jaccard is not None and not a.exact:
        sys.exit("[FAIL] neighbors: --min-jaccard is the floor of --exact; give that too")
    if a.exact and a.confirm:
        sys.exit("[FAIL] neighbors: --exact already reports the exact similarity; leave --confirm out")
    if a.exact and a.min_similarity is not None:
        sys.exit("[FAIL] neighbors: --min-similarity is a floor of the sketches; the floor of --exact is --min-jaccard")
    if a.min_jaccard is not None and not 0.0 < a.min_jaccard <= 1.0:      # NaN fails it too
        sys.exit(f"[FAIL] neighbors: --min-jaccard {a.min_jaccard} is outside (0, 1]")
    if a.pool_mb < 1 or a.counter_mb < 1:
        sys.exit("[FAIL] neighbors: --pool-mb and --counter-mb must be at least 1")
    if a.min_similarity is None:
        a.min_similarity = 1.0 / 64
    if not 1 <= a.k <= indexio.SIG_MAX_K:
        sys.exit(f"[FAIL] neighbors: -k {a.k} is outside 1..{indexio.SIG_MAX_K}")
    if a.tids is not None and not os.path.isfile(a.tids):
        print(f"[FAIL] {a.tids} not found", file=sys.stderr)
        sys.exit(2)
    prefixes, tids = _sig_plan(a, "neighbors")
    two = len(prefixes) == 2
    ids = None
    if a.tids is not None:
        try:
            with open(a.tids) as f:
                asked = [line.strip() for line in f if line.strip()]
        except (OSError, UnicodeDecodeError) as e:
            print(f"[FAIL] neighbors: unreadable input ({e})", file=sys.stderr)
            sys.exit(2)
        ids = np.unique(_ids_of_tids("neighbors", asked, a.tids, tids[0], a.index))
    thr64 = indexio.signature_threshold(a.min_similarity)
    try:
        ctx = None
        if not a.host:
            import folddisco_amd as fd
            ctx = fd.Context(a.device)
        if a.exact:
            return _neighbors_exact(a, ctx, prefixes, tids, ids)
        tabs = [_dups_signatures(a, ctx, p, len(t)) for p, t in zip(prefixes, tids)]
        A, D = tabs[0], (tabs[1] if two else tabs[0])
        if ids is None:
            ids = np.arange(len(A), dtype=np.int64)
            Q, cand, excl = A, (D if two else None), None
        else:                                        # chosen queries: against the whole table, each one's own id excluded inside one index
            Q, cand, excl = A[ids], D, (None if two else ids.astype(np.uint32))
        nb = indexio.signature_neighbors_host(Q, cand, k=a.k, thr64=thr64, exclude=excl, threads=a.threads) if a.host else \
            ctx.signature_neighbors(Q, cand, k=a.k, thr64=thr64, exclude=excl)
        at_q, at_r = np.nonzero(nb["id"] != indexio.SIG_NO_ID)       # row-major: ascending (id, rank)
        got = nb[at_q, at_r]
        jac = _dups_jaccard(a, ctx, prefixes, tids, ids[at_q], got["id"]) if a.confirm else None
    except (OSError, ValueError) as e:
        print(f"[FAIL] neighbors: {e}", file=sys.stderr)
        sys.exit(2 if isinstance(e, OSError) else 1)
    td = tids[1] if two else tids[0]
    lines = []
    for j, (q, rank, r) in enumerate(zip(at_q, at_r, got)):
        iq, ib = int(ids[q]), int(r["id"])
        cols = [str(iq), tids[0][iq], str(int(A["n"][iq])), str(int(rank) + 1), str(ib), td[ib], str(int(D["n"][ib])), str(int(r["match"])), str(int(r["filled"])),
                f"{int(r['match']) / int(r['filled']):.4f}", "identical" if int(r["flags"]) & indexio.SIG_IDENTICAL else "similar"]
        if jac is not None:
            cols.append(f"{jac[j]:.4f}")
        lines.append("\t".join(cols) + "\n")
    _write_tsv(a.output, lines, "neighbors")
    n_none = int((nb["id"][:, 0] == indexio.SIG_NO_ID).sum())
    n_ident = int(((nb["flags"][:, 0] & indexio.SIG_IDENTICAL) != 0).sum())
    print(f"[OK] {' x '.join(prefixes)}: {' x '.join(str(len(t)) for t in tids)} structures, k = {a.k}, {len(lines)} rows, {n_none} without a neighbour, "
          f"{n_ident} with an identical nearest, floor {thr64}/64")
    if a.verbose:
        print(f"[INFO] neighbors on the {'host' if a.host else 'device'}: {len(ids)} queries, signatures of {sum(len(t) for t in tids)} structures "
              f"({sum(t.nbytes for t in tabs)} bytes)" + (f", {len(jac)} rows confirmed from their rows" + _extractions(a) if jac is not None else ""), file=sys.stderr)


def _neighbors_exact(a, ctx, prefixes, tids, ids):
    """`neighbors --exact`: the k nearest of the structures `ids` (ascending; None: every structure) by the exact Jaccard similarity of their
    rows, from one walk over the posting lists of each query's hashes (indexio.row_neighbors on the device, row_neighbors_host with --host).
    Every index is loaded once: checked if --verify, its signatures taken for n and the row lengths of the database, then kept for the walk;
    inside one index a structure's own id is excluded.  A damaged index is a ValueError on either path.  One TSV row per neighbour, sorted by
    (id, rank): id tid n rank nb_id nb_tid nb_n inter union jaccard class"""
    from folddisco_amd import indexio
    two = len(prefixes) == 2
    T = 0 if a.min_jaccard is None else indexio.jaccard_floor(a.min_jaccard)
    pool, counter = a.pool_mb * (1 << 20) // 4, a.counter_mb * (1 << 20)
    files = [indexio.read_index_files(p) + (len(t),) for p, t in zip(prefixes, tids)]
    if a.host:
        if a.verify:
            for p, (v, h, o, n) in zip(prefixes, files):
                _stop_if_unsound(indexio.verify_host(v, h, o, n, threads=a.threads), p)
        tabs = [np.array(indexio.signatures_host(v, h, o, n, threads=a.threads)) for v, h, o, n in files]
    else:
        import folddisco_amd as fd
        ixs = [fd.FolddiscoIndex.load(ctx, h, o, v, n) for v, h, o, n in files]
        del files
        if a.verify:
            for p, ix in zip(prefixes, ixs):
                _stop_if_unsound(ix.verify(), p)
        tabs = [np.array(ix.signatures(window=a.window)) for ix in ixs]
    A, D = tabs[0], tabs[-1]
    ids = np.arange(len(A), dtype=np.int64) if ids is None else ids
    d_len = np.ascontiguousarray(D["n"], dtype=np.uint32)
    excl = None if two else ids.astype(np.uint32)
    if a.host:
        nb = indexio.row_neighbors_host(files[0], files[1] if two else None, ids, d_len, k=a.k, floor_e4=T, exclude=excl, window=a.window, pool_hashes=pool,
                                        threads=a.threads)
    else:
        try:
            nb = indexio.row_neighbors(ixs[0], ixs[1] if two else None, ids, d_len, k=a.k, floor_e4=T, exclude=excl, window=a.window, pool_hashes=pool,
                                       counter_bytes=counter)
        except fd.FdgpuError as e:                   # a damaged index: the [FAIL] line and status 1 of --host
            raise ValueError(str(e)) from None
    at_q, at_r = np.nonzero(nb["id"] != indexio.ROW_NO_ID)           # row-major: ascending (id, rank)
    td = tids[1] if two else tids[0]
    lines = []
    for q, rank, r in zip(at_q, at_r, nb[at_q, at_r]):
        iq, ib, inter, union = int(ids[q]), int(r["id"]), int(r["inter"]), int(r["union"])
        lines.append("\t".join([str(iq), tids[0][iq], str(int(A["n"][iq])), str(int(rank) + 1), str(ib), td[ib], str(int(D["n"][ib])), str(inter), str(union),
                                f"{inter / max(union, 1):.4f}", "identical" if int(r["flags"]) & indexio.ROW_EQUAL else "similar"]) + "\n")
    _write_tsv(a.output, lines, "neighbors")
    n_none = int((nb["id"][:, 0] == indexio.ROW_NO_ID).sum()) if len(ids) else 0
    n_ident = int(((nb["flags"][:, 0] & indexio.ROW_EQUAL) != 0).sum()) if len(ids) else 0
    print(f"[OK] {' x '.join(prefixes)}: {' x '.join(str(len(t)) for t in tids)} structures, k = {a.k}, exact, {len(lines)} rows, {n_none} without a neighbour, "
          f"{n_ident} with an identical nearest, floor {T}/10000")
    if a.verbose:
        print(f"[INFO] neighbors --exact on the {'host' if a.host else 'device'}: {len(ids)} queries against {len(D)} structures", file=sys.stderr)


def _cluster_seed_ids(a, tids2):
    """the seeds of `cluster --against`: the ids in PREFIX2 of the tids of --against-reps FILE, ascending, or every structure of PREFIX2
    without one.  Status 1 and a [FAIL] line for a tid PREFIX2.lookup does not hold or holds in several rows, status 2 for an unreadable file"""
    if a.against_reps is None:
        return np.arange(len(tids2), dtype=np.int64)
    try:
        with open(a.against_reps) as f:
            asked = list(dict.fromkeys(line.strip() for line in f if line.strip()))
    except (OSError, UnicodeDecodeError) as e:
        print(f"[FAIL] cluster: unreadable input ({e})", file=sys.stderr)
        sys.exit(2)
    ids = _ids_of_tids("cluster", asked, a.against_reps, tids2, a.against)
    if len(ids) != len(asked):
        rows = {}
        for t in tids2:
            rows[t] = rows.get(t, 0) + 1
        twice = [t for t in asked if rows[t] > 1]
        print(f"[FAIL] cluster: {len(twice)} tid(s) of {a.against_reps} name more than one row of {a.against}.lookup: " + ", ".join(twice[:10])
              + (" ..." if len(twice) > 10 else ""))
        sys.exit(1)
    return np.sort(ids)


def cmd_cluster(a):
    """`cluster`: a non-redundant subset of the index at PREFIX.  The signatures are taken as `dups` takes them and walked in the order of
    --rep-by (hashes: the signature's n, descending; nres, plddt: that column of PREFIX.lookup, descending; id: ascending; ties by id): a
    structure that no representative chosen so far is reported with at --min-similarity becomes a representative, any other joins its nearest
    one (the order of `neighbors`), on the device (fdgpu_signature_clusters) or with --host on the CPU (no device is opened).  One TSV row per
    structure with a non-empty row, sorted by (rep_id, id): rep_id rep_tid rep_n id tid n match filled estimate class[ jaccard]; class is
    `representative`, `identical` or `similar`.  --redundant FILE gets the members' tids, one per line in id order: what `update --remove`
    takes; it is refused when such a tid also names a kept row.  --min-jaccard F (implies --confirm) changes no cluster: it lists in --redundant
    only the members whose exact similarity with their representative reaches F; a member below it is kept, and counts among the kept rows of
    that refusal.  --representatives FILE gets the representatives' tids, one per line in id order.  It removes nothing itself.  No structure
    file is read.
    --against PREFIX2: the structures of PREFIX2 (or, with --against-reps FILE, those whose tids the file lists) are representatives before
    the walk starts (fdgpu_signature_clusters_seeded): which structures of PREFIX are new?  A structure joins the nearest of the seeds and the
    representatives chosen from PREFIX; on a full tie a seed wins.  The rows gain a column rep_from after class, `against` (rep_id, rep_tid and
    rep_n are those of PREFIX2) or `self`, and are sorted by (against before self, rep_id, id); a seed gets no row.  --confirm intersects the
    members of seeds across the two indices.  --redundant lists the members of either kind, --representatives the new representatives only:
    appended to the list the seeds came from, it is the next --against-reps."""
    from folddisco_amd import indexio
    if a.rep_by not in indexio.CLUSTER_ORDER_KEYS:
        print(f"[FAIL] cluster: unknown --rep-by key '{a.rep_by}' (one of {', '.join(indexio.CLUSTER_ORDER_KEYS)})")
        sys.exit(1)
    if a.against is not None and os.path.abspath(a.against) == os.path.abspath(a.index):
        # status 2, not the 1 of `dups`: before `cluster` had the flag this command line ended with the parser's status 2, and it keeps it
        print(f"[FAIL] cluster: --against {a.against} is the index itself; leave it out to cluster inside one index", file=sys.stderr)
        sys.exit(2)
    if a.against_reps is not None:
        if a.against is None:
            sys.exit("[FAIL] cluster: --against-reps lists structures of --against PREFIX2; give that too")
        if not os.path.isfile(a.against_reps):
            print(f"[FAIL] {a.against_reps} not found", file=sys.stderr)
            sys.exit(2)
    _min_jaccard_plan(a, "cluster")
    prefixes, all_tids = _sig_plan(a, "cluster")
    prefix, tids = prefixes[0], all_tids[0]
    two = len(prefixes) == 2
    seed_ids = _cluster_seed_ids(a, all_tids[1]) if two else None
    thr64 = indexio.signature_threshold(a.min_similarity)
    try:
        rows = indexio.read_lookup_rows(prefix + ".lookup") if a.rep_by in ("nres", "plddt") else None
        ctx = None
        if not a.host:
            import folddisco_amd as fd
            ctx = fd.Context(a.device)
        S = _dups_signatures(a, ctx, prefix, len(tids))
        S2 = _dups_signatures(a, ctx, prefixes[1], len(all_tids[1])) if two else None
        seeds = np.ascontiguousarray(S2[seed_ids]) if two else None
        order = indexio.cluster_order(S, rows, a.rep_by)
        cl = indexio.signature_clusters_host(S, order, thr64=thr64, threads=a.threads, seeds=seeds) if a.host else \
            ctx.signature_clusters(S, order, thr64=thr64, seeds=seeds)
        ids = np.arange(len(S), dtype=np.int64)
        of_seed = (cl["flags"] & indexio.SIG_SEED) != 0                       # the record's id is a position among the seeds
        rep = ~of_seed & (cl["id"] == ids)
        member = ~rep & (cl["id"] != indexio.SIG_NO_ID)
        rep_id = cl["id"].astype(np.int64)                                    # in PREFIX2 for a member of a seed, in PREFIX otherwise
        if two:
            rep_id[of_seed] = seed_ids[rep_id[of_seed]]
        def refuse_clash(listed_rows):               # `update --remove` removes every row with a listed tid: none of them may name a kept row
            listed = {tids[p] for p in ids[listed_rows]}
            clash = sorted({tids[p] for p in ids[~listed_rows] if tids[p] in listed})
            if clash:
                print(f"[FAIL] cluster: {len(clash)} tid(s) of --redundant also name a structure that is kept, and `update --remove` would remove that one too: "
                      + ", ".join(clash[:10]) + (", ..." if len(clash) > 10 else ""))
                sys.exit(1)
        removable, n_below = member, 0               # the rows --redundant lists
        if a.redundant and a.min_jaccard is None:
            refuse_clash(removable)
        shown = ids[rep | member]
        shown = shown[np.lexsort((shown, rep_id[shown], ~of_seed[shown]))]
        jac = None
        if a.confirm:
            mem = shown[member[shown]]
            if two:                                  # members of seeds across the two indices, members of new representatives inside PREFIX
                ms, mn = mem[of_seed[mem]], mem[~of_seed[mem]]
                across = _dups_overlaps(a, ctx, prefixes, all_tids, ms, rep_id[ms])
                st = dict(a.overlap_stats)
                inside = _dups_overlaps(a, ctx, prefixes[:1], [tids], rep_id[mn], mn)
                a.overlap_stats = {k: st[k] + v for k, v in a.overlap_stats.items()}
                exact = tuple(np.concatenate(x) for x in zip(across, inside))      # in the order of mem: the seeds' members come first
            else:
                exact = _dups_overlaps(a, ctx, prefixes, [tids], cl["id"][mem], mem)
            jac = _jaccard_values(exact)
            if a.min_jaccard is not None:            # a member below the exact floor is kept: keeping a redundant structure is harmless, deleting a distinct one is not
                below = ~indexio.jaccard_reaches(exact[0], exact[1] + exact[2] - exact[0], a.min_jaccard)
                removable = member.copy()
                removable[mem[below]] = False
                n_below = int(below.sum())
                if a.redundant:
                    refuse_clash(removable)
    except (OSError, ValueError) as e:
        print(f"[FAIL] cluster: {e}", file=sys.stderr)
        sys.exit(2 if isinstance(e, OSError) else 1)
    lines, j = [], 0
    for p in shown:
        r, rec = int(rep_id[p]), cl[p]
        rt, rs = (all_tids[1], S2) if of_seed[p] else (tids, S)
        cols = [str(r), rt[r], str(int(rs["n"][r])), str(int(p)), tids[p], str(int(S["n"][p])), str(int(rec["match"])), str(int(rec["filled"])),
                f"{int(rec['match']) / max(int(rec['filled']), 1):.4f}",
                "representative" if rep[p] else "identical" if int(rec["flags"]) & indexio.SIG_IDENTICAL else "similar"]
        if two:
            cols.append("against" if of_seed[p] else "self")
        if jac is not None:
            cols.append("1.0000" if rep[p] else f"{jac[j]:.4f}")
            j += 0 if rep[p] else 1
        lines.append("\t".join(cols) + "\n")
    _write_tsv(a.output, lines, "cluster")
    if a.redundant:
        _write_tsv(a.redundant, [tids[p] + "\n" for p in ids[removable]], "cluster")
    if a.representatives:
        _write_tsv(a.representatives, [tids[p] + "\n" for p in ids[rep]], "cluster")
    own = shown[~of_seed[shown]]                                              # the rows of the clusters PREFIX itself started
    sizes = np.bincount(rep_id[own], minlength=max(len(S), 1))
    n_ident = int((member & ((cl["flags"] & indexio.SIG_IDENTICAL) != 0)).sum())
    n_none = int((cl["id"] == indexio.SIG_NO_ID).sum())
    floor = f", {n_below} members below the exact floor kept" if a.min_jaccard is not None else ""
    if two:
        print(f"[OK] {prefix} x {prefixes[1]}: {len(S)} x {len(S2)} structures, {len(seed_ids)} seeds, {int(rep.sum())} new clusters "
              f"({int((sizes[ids[rep]] == 1).sum())} singletons), {int((member & of_seed).sum())} members of seeds, {int((member & ~of_seed).sum())} members of new "
              f"representatives ({n_ident} identical), {n_none} unclustered, threshold {thr64}/64" + floor)
    else:
        print(f"[OK] {prefix}: {len(S)} structures, {int(rep.sum())} clusters ({int((sizes[ids[rep]] == 1).sum())} singletons), {int(member.sum())} members "
              f"({n_ident} identical), {n_none} unclustered, largest cluster {int(sizes.max())}, threshold {thr64}/64" + floor)
    if a.verbose:
        print(f"[INFO] cluster on the {'host' if a.host else 'device'}: signatures of {len(S)} structures ({S.nbytes} bytes), walked by {a.rep_by}"
              + (f", {len(seed_ids)} seeds of {prefixes[1]} ({int((seeds['n'] == 0).sum())} of them with empty rows)" if two else "")
              + (f", {len(jac)} members confirmed from their rows" + _extractions(a) if jac is not None else ""), file=sys.stderr)


def _reshard_plan(a):
    """everything `reshard` decides before it opens a device: -> (source prefixes, structures).  Status 2 for missing or unreadable files,
    status 1 and a [FAIL] line for a refusal; nothing is written in either case."""
    from folddisco_amd import indexio
    for name, w in (("--from", a.from_), ("--to", a.to)):
        if not 1 <= w <= 64:
            sys.exit(f"[FAIL] reshard: {name} {w} is outside 1..64")
    if a.from_ == a.to:
        sys.exit(f"[FAIL] reshard: --from and --to are both {a.to}: nothing to do")
    srcs = [a.index] if a.from_ == 1 else [_shard_prefix(a.index, k, a.from_) for k in range(a.from_)]
    need = [a.index + ".lookup", a.index + ".type"] + [s + ext for s in srcs for ext in ("", ".offset")]
    for f in need:
        if not os.path.isfile(f):
            print(f"[FAIL] {f} not found", file=sys.stderr)
            sys.exit(2)
    try:
        bad, n = indexio.check_lookup_type(a.index)
        for s in srcs:
            bad += indexio.check_value_offset_pair(s)
    except (OSError, ValueError, UnicodeDecodeError) as e:
        print(f"[FAIL] {a.index}: unreadable ({e})", file=sys.stderr)
        sys.exit(2)
    if bad:
        print("[FAIL] index files are inconsistent: " + "; ".join(bad))
        sys.exit(1)
    return srcs, n


def cmd_reshard(a):
    """`reshard`: the index at PREFIX (--from 1) or its shards PREFIX.shard<k>ofV (--from V) rewritten as W shards by structure id range
    (--to W: OUT.shard<r>ofW, the ranges of indexio.shard_bounds, ids absolute — what a W-rank `query` reads) or as the single index (--to 1).
    Shards are merged and cut on the device (fdgpu_index_merge, fdgpu_index_split) or with --host on the CPU (no device is opened).  Files are
    written under temporary names and renamed at the end; shard files of another count are left alone."""
    import shutil
    from folddisco_amd import indexio
    srcs, S = _reshard_plan(a)
    V, W = a.from_, a.to
    out = a.output or a.index
    # a store is checked against the single index's files only (--from 1); beside shards its stamp cannot be checked and it is copied as it is
    store = _open_store(a.index + ".coords", a.index if V == 1 else None, S) if out != a.index and os.path.isfile(a.index + ".coords") else None
    try:
        loaded = [indexio.read_index_files(s) for s in srcs]
    except (OSError, ValueError) as e:
        print(f"[FAIL] {a.index}: unreadable ({e})", file=sys.stderr)
        sys.exit(2)
    src_b, dst_b = indexio.shard_bounds(V, S), indexio.shard_bounds(W, S)
    if a.host:
        if a.verify:
            for k, (v, h, o) in enumerate(loaded):
                _stop_if_unsound(indexio.verify_host(v, h, o, int(src_b[k + 1] - src_b[k]), first_id=int(src_b[k]), threads=a.threads), srcs[k])
        whole = loaded[0] if V == 1 else indexio.merge_subindices(loaded)
        del loaded
        parts = [whole] if W == 1 else indexio.split_host(*whole, bounds=dst_b, first_id=0, threads=a.threads)
        if a.verify:
            for r, (v, h, o) in enumerate(parts):
                _stop_if_unsound(indexio.verify_host(v, h, o, int(dst_b[r + 1] - dst_b[r]), first_id=int(dst_b[r]), threads=a.threads),
                                 f"part {r} of the result; nothing was written")
        stats = [(len(h), int(np.count_nonzero(v < 128)), len(v)) for v, h, o in parts]      # a posting ends at every byte without the continuation bit
        save = [lambda p, x=x: indexio.write_index_files(p, *x) for x in parts]
    else:
        import folddisco_amd as fd
        ctx = fd.Context(a.device)
        res = [fd.FolddiscoIndex.load(ctx, h, o, v, int(src_b[k + 1] - src_b[k]), first_id=int(src_b[k])) for k, (v, h, o) in enumerate(loaded)]
        del loaded
        if a.verify:
            for k, ix in enumerate(res):
                _stop_if_unsound(ix.verify(), srcs[k])
        whole = res[0] if V == 1 else fd.FolddiscoIndexSet(res).merge()
        del res
        parts = [whole] if W == 1 else whole.split(dst_b)
        if a.verify:
            for r, ix in enumerate(parts):
                _stop_if_unsound(ix.verify(), f"part {r} of the result; nothing was written")
        stats = [(ix.num_hashes, ix.num_postings, ix.value_len) for ix in parts]
        save = [ix.save for ix in parts]
    finals = [out] if W == 1 else [_shard_prefix(out, r, W) for r in range(W)]
    side = [".lookup", ".type"] if out != a.index else []
    tmp = f"{out}.reshard-tmp{os.getpid()}"
    made = []
    try:
        for r, (fin, sv) in enumerate(zip(finals, save)):
            sv(f"{tmp}.{r}")
            made += [(f"{tmp}.{r}{ext}", fin + ext) for ext in ("", ".offset")]
        for ext in side:
            shutil.copyfile(a.index + ext, tmp + ext)
            made.append((tmp + ext, out + ext))
        if side and store is not None:           # the store covers the whole database: it goes with .lookup; its stamp is re-taken where a single index is written
            if W == 1:
                indexio.write_coords(tmp + ".coords", [(store, None)], _tmp_stamp(f"{tmp}.0", S))
            else:
                shutil.copyfile(a.index + ".coords", tmp + ".coords")
            made.append((tmp + ".coords", out + ".coords"))
        for t, f in made:
            os.replace(t, f)
    finally:
        for t, _ in made:
            if os.path.exists(t):
                os.remove(t)
        for r in range(len(finals)):
            for ext in ("", ".offset"):
                if os.path.exists(f"{tmp}.{r}{ext}"):
                    os.remove(f"{tmp}.{r}{ext}")
    per = ", ".join(f"{h} / {p} / {b}" for h, p, b in stats)
    print(f"[OK] {a.index}: {V} -> {W}, {S} structures, per part lists / postings / bytes: {per}")
    if a.verbose:
        print(f"[INFO] wrote {', '.join(finals)}" + (f" and copied .lookup / .type to {out}" if side else "") + f"; merged and cut on the {'host' if a.host else 'device'}; "
              f"shard files of a count other than {W} are left as they are", file=sys.stderr)


def _merge_plan(a):
    """everything `merge` decides before it opens a device: -> (lookup rows per input, type text of the first input, Foldcomp-built?).  Status 2
    for missing or unreadable files, status 1 and a [FAIL] line for a refusal; nothing is written in either case."""
    from folddisco_amd import indexio
    if not 2 <= len(a.index) <= 64:
        sys.exit(f"[FAIL] merge: {len(a.index)} input(s) given, 2 to 64 are joined in one call")
    if not a.output:
        sys.exit("[FAIL] merge: -o/--output is required")
    if os.path.abspath(a.output) in [os.path.abspath(p) for p in a.index]:
        sys.exit(f"[FAIL] merge: the output {a.output} is one of the inputs")
    for p in a.index:
        for ext in INDEX_FILES:
            if not os.path.isfile(p + ext):
                print(f"[FAIL] {p}{ext} not found", file=sys.stderr)
                sys.exit(2)
    try:
        bad = [b for p in a.index for b in indexio.check_index_files(p)]
        rows = [indexio.read_lookup_rows(p + ".lookup") for p in a.index]
        texts = []
        for p in a.index:
            with open(p + ".type") as f:
                texts.append(f.read())
    except (OSError, ValueError, UnicodeDecodeError) as e:
        print(f"[FAIL] merge: unreadable input ({e})", file=sys.stderr)
        sys.exit(2)
    if bad:
        print("[FAIL] index files are inconsistent: " + "; ".join(bad))
        sys.exit(1)
    key = indexio.check_joinable(texts)
    if key is not None:
        print(f"[FAIL] merge: the inputs' .type files differ in {key}: indices are joined only if they were built with the same settings"
              + (" from the same kind of input" if key in ("input_format", "foldcomp_db") else ""))
        sys.exit(1)
    have = [os.path.isfile(p + ".coords") for p in a.index]
    if any(have) and not all(have):
        print("[FAIL] merge: only some inputs have a coordinate store; without one: " + ", ".join(p for p, h in zip(a.index, have) if not h) +
              " (run `coords -i PREFIX` on them, or remove the others' .coords files)")
        sys.exit(1)
    a.stores = [_open_store(p + ".coords", p, len(r)) for p, r in zip(a.index, rows)] if all(have) else None
    total = sum(len(r) for r in rows)
    if total > 0xffffffff:
        print(f"[FAIL] merge: {total} structures in all, structure ids are 32 bits")
        sys.exit(1)
    return rows, texts[0], indexio.load_type(a.index[0] + ".type").get("input_format") == "FCZDB"


def cmd_merge(a):
    """`merge`: indices that were built separately (each with ids from 0) joined into one, byte for byte what `index` writes over the first
    input's structures in their order followed by the second's and so on.  Every input is loaded, moved to the running structure count
    (fdgpu_index_rebase) and released; the moved parts are concatenated per hash on the device (fdgpu_index_merge), or with --host both steps run
    on the CPU (fdgpu_rebase_host, fdgpu_merge_subindices; no device is opened).  No structure file is read.  The four files are written under
    temporary names and renamed at the end."""
    from folddisco_amd import indexio
    rows, type_text, fczdb = _merge_plan(a)
    counts = [len(r) for r in rows]
    S, out = sum(counts), a.output
    try:
        if a.host:
            parts, first = [], 0
            for p, n in zip(a.index, counts):
                v, h, o = indexio.read_index_files(p)
                if a.verify:
                    _stop_if_unsound(indexio.verify_host(v, h, o, n, threads=a.threads), p)
                parts.append(indexio.rebase_host(v, h, o, 0, first, n, threads=a.threads) if first else (v, h, o))
                first += n
            v, h, o = indexio.merge_subindices(parts)
            del parts
            if a.verify:
                _stop_if_unsound(indexio.verify_host(v, h, o, S, threads=a.threads), "the joined index; nothing was written")
            stats = (len(h), int(np.count_nonzero(v < 128)), len(v))      # a posting ends at every byte without the continuation bit
            save = lambda prefix: indexio.write_index_files(prefix, v, h, o)
        else:
            import folddisco_amd as fd
            ctx = fd.Context(a.device)
            parts, first = [], 0
            for p, n in zip(a.index, counts):
                v, h, o = indexio.read_index_files(p)
                ix = fd.FolddiscoIndex.load(ctx, h, o, v, n)
                del v, h, o
                if a.verify:                     # before the rebase or the merge uses its offsets as addresses
                    _stop_if_unsound(ix.verify(), p)
                parts.append(ix.rebase(first) if first else ix)      # the loaded index is released once its moved copy exists
                del ix
                first += n
            whole = fd.FolddiscoIndexSet(parts).merge()
            del parts
            if a.verify:
                _stop_if_unsound(whole.verify(), "the joined index; nothing was written")
            stats = (whole.num_hashes, whole.num_postings, whole.value_len)
            save = whole.save
    except (OSError, ValueError) as e:
        print(f"[FAIL] merge: {e}", file=sys.stderr)
        sys.exit(2 if isinstance(e, OSError) else 1)
    tmp = f"{out}.merge-tmp{os.getpid()}"
    exts = INDEX_FILES + ((".coords",) if a.stores else ())
    try:
        save(tmp)
        with open(tmp + ".lookup", "w", newline="") as f:
            f.writelines(indexio.join_lookup_rows(rows, keep_db_keys=fczdb))
        with open(tmp + ".type", "w") as f:
            f.write(indexio.update_type_text(type_text, S))
        if a.stores:                             # the inputs' stores one after the other, like their .lookup rows
            indexio.write_coords(tmp + ".coords", [(st, None) for st in a.stores], _tmp_stamp(tmp, S))
        for ext in exts:
            os.replace(tmp + ext, out + ext)
    finally:
        for ext in exts:
            if os.path.exists(tmp + ext):
                os.remove(tmp + ext)
    print(f"[OK] {out}: {len(a.index)} inputs, {S} structures, lists / postings / bytes: {stats[0]} / {stats[1]} / {stats[2]}")
    if a.verbose:
        tids = [r.rstrip("\n").split("\t")[1] for rs in rows for r in rs]
        print(f"[INFO] joined {', '.join(f'{p} ({n})' for p, n in zip(a.index, counts))} on the {'host' if a.host else 'device'}; "
              f"{len(tids) - len(set(tids))} duplicate tid(s) across the inputs, kept as they are", file=sys.stderr)


def _reorder_plan(a):
    """everything `reorder` decides before it opens a device: -> (lookup rows, new_id, Foldcomp-built?).  Status 2 for missing or unreadable files,
    status 1 and a [FAIL] line for a refusal; nothing is written in either case."""
    from folddisco_amd import indexio
    if (a.by is None) == (a.order is None):
        sys.exit("[FAIL] reorder: give exactly one of --by KEY and --order FILE")
    if a.by is not None and a.by not in indexio.ORDER_KEYS:
        sys.exit(f"[FAIL] reorder: unknown --by key '{a.by}' (one of {', '.join(indexio.ORDER_KEYS)})")
    need = [a.index + ext for ext in INDEX_FILES] + ([a.order] if a.order is not None else [])
    for f in need:
        if not os.path.isfile(f):
            print(f"[FAIL] {f} not found", file=sys.stderr)
            sys.exit(2)
    try:
        bad = indexio.check_index_files(a.index)
        rows = indexio.read_lookup_rows(a.index + ".lookup")
        fczdb = indexio.load_type(a.index + ".type").get("input_format") == "FCZDB"
        order_tids = None
        if a.order is not None:
            with open(a.order, newline="") as f:
                order_tids = [line.rstrip("\r\n") for line in f]
            while order_tids and not order_tids[-1]:      # blank lines at the end of the file
                order_tids.pop()
    except (OSError, ValueError, UnicodeDecodeError) as e:
        print(f"[FAIL] reorder: unreadable input ({e})", file=sys.stderr)
        sys.exit(2)
    if bad:
        print("[FAIL] index files are inconsistent: " + "; ".join(bad))
        sys.exit(1)
    try:
        new_id = indexio.order_from_lookup(rows, by=a.by, descending=a.desc, order_tids=order_tids)
    except ValueError as e:
        print(f"[FAIL] reorder: {e}")
        sys.exit(1)
    a.store = _open_store(a.index + ".coords", a.index, len(rows)) if os.path.isfile(a.index + ".coords") else None      # a stale store is refused here
    return rows, new_id, fczdb


def cmd_reorder(a):
    """`reorder`: the index at PREFIX with its structures in another order (--by tid|nres|plddt [--desc]: PREFIX.lookup sorted by one column,
    stably; --order FILE: one tid per line), byte for byte what `index` writes over the structures in the new order.  Every posting list is
    decoded, mapped, put back in ascending order and re-encoded on the device (fdgpu_index_permute), or with --host on the CPU
    (fdgpu_permute_host; no device is opened).  No structure file is read.  PREFIX.type is copied unchanged; the four files are written under
    temporary names and renamed at the end."""
    import shutil
    from folddisco_amd import indexio
    rows, new_id, fczdb = _reorder_plan(a)
    S, out = len(rows), a.output or a.index
    try:
        v, h, o = indexio.read_index_files(a.index)
        before = len(v)
        if a.host:
            if a.verify:
                _stop_if_unsound(indexio.verify_host(v, h, o, S, threads=a.threads), a.index)
            v, h, o = indexio.permute_host(v, h, o, new_id, threads=a.threads)
            if a.verify:
                _stop_if_unsound(indexio.verify_host(v, h, o, S, threads=a.threads), "the reordered index; nothing was written")
            stats = (len(h), int(np.count_nonzero(v < 128)), len(v))      # a posting ends at every byte without the continuation bit
            save = lambda prefix: indexio.write_index_files(prefix, v, h, o)
        else:
            import folddisco_amd as fd
            ctx = fd.Context(a.device)
            src = fd.FolddiscoIndex.load(ctx, h, o, v, S)
            del v, h, o
            if a.verify:                             # before the permute uses its offsets and ids as addresses
                _stop_if_unsound(src.verify(), a.index)
            ix = src.permute(new_id)
            del src
            if a.verify:
                rep = ix.verify()
                _stop_if_unsound(rep, "the reordered index; nothing was written")
            stats = (ix.num_hashes, ix.num_postings, ix.value_len)
            save = ix.save
    except (OSError, ValueError) as e:
        print(f"[FAIL] reorder: {e}", file=sys.stderr)
        sys.exit(2 if isinstance(e, OSError) else 1)
    tmp = f"{out}.reorder-tmp{os.getpid()}"
    exts = INDEX_FILES + ((".coords",) if a.store is not None else ())
    try:
        save(tmp)
        with open(tmp + ".lookup", "w", newline="") as f:
            f.writelines(indexio.permute_lookup_rows(rows, new_id, keep_db_keys=fczdb))
        shutil.copyfile(a.index + ".type", tmp + ".type")
        if a.store is not None:                  # position p of the result holds the structure that was at argsort(new_id)[p]
            indexio.write_coords(tmp + ".coords", [(a.store, np.argsort(new_id, kind="stable"))], _tmp_stamp(tmp, S))
        for ext in exts:
            os.replace(tmp + ext, out + ext)
    finally:
        for ext in exts:
            if os.path.exists(tmp + ext):
                os.remove(tmp + ext)
    moved = int(np.count_nonzero(new_id != np.arange(S, dtype=np.uint32)))
    print(f"[OK] {out}: {S} structures reordered ({moved} moved), lists / postings / bytes: {stats[0]} / {stats[1]} / {stats[2]}")
    if a.verbose:
        print(f"[INFO] reordered {a.index} {'by ' + a.by + (' (descending)' if a.desc else '') if a.by else 'as ' + a.order + ' says'} on the "
              f"{'host' if a.host else 'device'}; value bytes {before} -> {stats[2]}", file=sys.stderr)


def _coords_plan(a):
    """everything `coords` decides before it parses a structure: -> (keys or paths in id order, Foldcomp database or None, rows).  Status 2 for missing
    or unreadable index files, status 1 and a [FAIL] line for a refusal; nothing is written in either case."""
    from folddisco_amd import indexio, structure
    for ext in INDEX_FILES:
        if not os.path.isfile(a.index + ext):
            print(f"[FAIL] {a.index}{ext} not found", file=sys.stderr)
            sys.exit(2)
    try:
        bad, n = indexio.check_lookup_type(a.index)
        tids, _nres, _plddt, db_keys = indexio.load_lookup(a.index + ".lookup") if not bad else ([], None, None, None)
        cfg = indexio.load_type(a.index + ".type") if not bad else {}
    except (OSError, ValueError, IndexError, UnicodeDecodeError) as e:
        print(f"[FAIL] {a.index}: unreadable ({e})", file=sys.stderr)
        sys.exit(2)
    if bad:
        print("[FAIL] index files are inconsistent: " + "; ".join(bad))
        sys.exit(1)
    if cfg.get("input_format") == "FCZDB":       # the database the index names, else the prefix's X_foldcomp sibling — as `query` finds it
        cands = [cfg.get("foldcomp_db", "")]
        pfx = a.index[:-len("_folddisco")] if a.index.endswith("_folddisco") else a.index
        cands += [pfx, pfx + "_foldcomp"]
        dbp = next((c for c in cands if c and structure.is_foldcomp_db(c)), None)
        if dbp is None:
            print(f"[FAIL] coords: Foldcomp database of index {a.index} not found (tried {', '.join(c for c in cands if c)})")
            sys.exit(1)
        fc = structure.FoldcompDb(dbp)
        known = set(int(k) for k in fc.keys)
        missing = [str(int(k)) for k in db_keys if int(k) not in known]
        what, items = "database keys", db_keys
    else:
        fc = None
        items = [_resolve_tid(a.index, t) for t in tids]
        missing = [p for p in items if not os.path.isfile(p)]
        what = "structure files"
    if missing:                                  # a store with silent holes would change results
        print(f"[FAIL] coords: {len(missing)} of the {n} {what} {a.index}.lookup names are missing: " + ", ".join(missing[:10]) + (" ..." if len(missing) > 10 else ""))
        sys.exit(1)
    return items, fc, n


def cmd_coords(a):
    """`coords`: PREFIX.coords for an existing index (built here, by the reference or by a multi-rank run): the structures PREFIX.lookup names,
    found as `query` finds them, parsed in chunks exactly as `index` parses them (a structure `index` skips keeps its slot with no residues) and
    streamed through indexio.write_coords.  No device is opened."""
    from folddisco_amd import indexio, structure
    items, fc, n = _coords_plan(a)
    out = a.output or a.index + ".coords"
    a.fc, a.fc_keys = fc, (np.asarray(items, np.uint64) if fc is not None else None)
    got = []
    a.coord_sink = got.append

    def pieces():
        for c0 in range(0, n, a.chunk):
            _ingest(a, structure, items[c0:c0 + a.chunk], c0)
            yield got.pop()
    indexio.write_coords(out, pieces(), lambda: indexio.index_stamp(a.index))
    st = indexio.CoordStore.open(out, check_prefix=a.index)
    print(f"[OK] {out}: {st.n_struct} structures, {st.n_res} residues, {os.path.getsize(out)} bytes")
    if a.verbose:
        print(f"[INFO] stamp: {', '.join(f'{k} = {v}' for k, v in zip(indexio.STAMP_FIELDS, st.stamp))}", file=sys.stderr)


def _resolve_tid(index, t):
    """a tid of PREFIX.lookup -> the structure file, like resolve_tid_path_from_index_prefix (controller/io.rs:488-528)"""
    if os.path.isfile(t):
        return t
    cand = os.path.join(os.path.dirname(os.path.abspath(index)), t)
    return cand if os.path.isfile(cand) else t


def cmd_query(a):
    import folddisco_amd as fd
    from folddisco_amd import indexio, query, structure
    if not a.index:
        sys.exit("[FAIL] -i/--index is required")
    if a.coords and a.no_coords:
        sys.exit("[FAIL] --coords and --no-coords cannot be combined")
    rank, world, dev = _init_dist(a)
    if a.verify and world == 1:
        _verify_files(a.index)
    tids, nres, plddt, db_keys = indexio.load_lookup(a.index + ".lookup")
    cfg = indexio.load_type(a.index + ".type")
    # the coordinate store (PREFIX.coords, or --coords FILE) replaces the parse of every structure file; --no-coords keeps the parse.  A store the
    # reader refuses ends the command here, before a device is opened: falling back to the files would hide that it is stale
    store = None
    store_path = a.coords or (a.index + ".coords" if os.path.isfile(a.index + ".coords") else "")
    if store_path and not a.no_coords and not a.skip_match:
        store = _open_store(store_path, a.index if world == 1 else None, len(tids))
        if a.verbose:
            print(f"[INFO] coordinates from {store_path}: {store.n_struct} structures, {store.n_res} residues" +
                  ("" if world == 1 else "; sharded query: the stamp is that of the single index's files and is not checked"), file=sys.stderr)
    ctx = fd.Context(a.device)
    shard = None
    lo, hi = 0, len(tids)
    if world > 1:
        # query sharded by structure id: this rank loads its shard of the index (written by the multi-rank index build) and the
        # coordinates of its own structures; ids in the shard are absolute, so it is loaded over the whole id range
        from folddisco_amd import dist as fdist
        sp = _shard_prefix(a.index, rank, world)
        if not os.path.exists(sp + ".offset"):
            sys.exit(f"[FAIL] {sp}.offset not found: build the index with the same number of ranks")
        lo, hi = fdist.shard_range(rank, world, len(tids))
        v, h, o = indexio.read_index_files(sp)
        ix = fd.FolddiscoIndex.load(ctx, h, o, v, len(tids))
        shard = dict(lo=lo, n_local=hi - lo, device=dev if os.environ.get("FD_BENCH_BACKEND", "nccl") == "nccl" else None, absolute=True)
    else:
        v, h, o = indexio.read_index_files(a.index)
        ix = fd.FolddiscoIndex.load(ctx, h, o, v, len(tids))
    if a.verify:                                 # before any scoring kernel sees the bytes
        _stop_if_unsound(ix.verify(), a.index if world == 1 else sp)
    if a.query.endswith((".txt", ".tsv")):
        queries = []
        for line in open(a.query):
            p = line.rstrip("\n").split("\t")
            queries.append((p[0], p[1] if len(p) > 1 else "", p[2] if len(p) > 2 else ""))
    else:
        queries = [(a.pdb, a.query, a.output)]
    # candidate coordinates: resolve tids like resolve_tid_path_from_index_prefix (controller/io.rs:488-528)
    resolve = lambda t: _resolve_tid(a.index, t)
    db_structs, batch = None, None
    # an index built from a Foldcomp database reads the hit coordinates back from it by db_key (query_pdb.rs:321-343,
    # retrieve.rs:166-178); the database is the one the index names, else INDEX-PREFIX's X_foldcomp sibling (controller/io.rs:422-448)
    fc = None
    if cfg.get("input_format") == "FCZDB" and not a.skip_match and store is None:
        cands = [cfg.get("foldcomp_db", "")]
        pfx = a.index[:-len("_folddisco")] if a.index.endswith("_folddisco") else a.index
        cands += [pfx, pfx + "_foldcomp"]
        dbp = next((c for c in cands if c and structure.is_foldcomp_db(c)), None)
        if dbp is None:
            sys.exit(f"[FAIL] Foldcomp database of index {a.index} not found (tried {', '.join(c for c in cands if c)})")
        fc = structure.FoldcompDb(dbp)
    if store is not None:                        # this rank's id range [lo, hi) of the store: views of the mapping, no structure file is opened
        batch = ctx.upload(store.slice(lo, hi).ps)
        db_structs = store.structs(lo, hi)
    elif not a.skip_match and fc is not None:
        db_structs, _ = structure.read_compact_structures(db_keys[lo:hi], threads=a.threads, foldcomp=fc)
        batch = ctx.upload(fd.PackedStructures.concat([s.as_item() for s in db_structs]))
    elif not a.skip_match:
        db_structs, _ = structure.read_compact_structures([resolve(t) for t in tids[lo:hi]], threads=a.threads)
        batch = ctx.upload(fd.PackedStructures.concat([s.as_item() for s in db_structs]))
    dthr = [float(x) for x in a.distance.replace(" ", "").split(",") if x]
    athr = [float(x) for x in a.angle.replace(" ", "").split(",") if x]
    for pdb, qstr, outp in queries:
        if ":" in pdb and not os.path.isfile(pdb):       # DB:NAME = an entry of a Foldcomp database as the query (controller/io.rs:303-333)
            qdb = structure.FoldcompDb(pdb.split(":")[0])
            q = structure.read_compact_structures([qdb.key_of(pdb.split(":")[1])], threads=1, foldcomp=qdb)[0][0]
        else:
            q = structure.read_compact_structures([pdb], threads=1)[0][0]
        rows, matches = query.query_pdb(ctx, ix, batch, db_structs, tids, nres, plddt, q, qstr, dist_thr=dthr, angle_thr=athr,
                                        ca_distance=a.ca_distance, top_n=a.top, skip_match=a.skip_match, serial_query=a.serial_index,
                                        freq_filter=a.freq_filter, length_penalty_power=0.5 if a.length_penalty is None else a.length_penalty,
                                        dist_cutoff=float(cfg.get("grid_width", 20.0)), nbin_dist=int(cfg.get("num_bin_dist", 0)),
                                        nbin_angle=int(cfg.get("num_bin_angle", 0)), hash_type=hash_type_index(cfg.get("hash_type", "PDBTrRosetta")), multiple_bins=cfg.get("multiple_bin"), sampling_ratio=a.sampling_ratio,
                                        sampling_count=a.sampling_count, sort_by=a.sort_by, partial_fit=a.partial_fit, skip_ca_match=a.skip_ca_match, match_top_n=1000 if a.web else "same", db_keys=db_keys,
                                        filters=dict(total_match=a.total_match, covered_node=a.covered_node, covered_node_ratio=a.covered_node_ratio,
                                                     max_node=a.max_node, max_node_ratio=a.max_node_ratio, score=a.score,
                                                     connected_node=a.connected_node, connected_node_ratio=a.connected_node_ratio,
                                                     num_residue=a.num_residue, plddt=a.plddt, rmsd=a.rmsd, tm_score=a.tm_score,
                                                     gdt_ts=a.gdt_ts, gdt_ha=a.gdt_ha, chamfer=a.chamfer, hausdorff=a.hausdorff),
                                        shard=shard)
        if rank != 0:
            continue                      # every rank holds the same result; rank 0 prints
        fh = open(outp, "w") if outp else sys.stdout
        if (a.skip_match or a.per_structure) and not a.web:      # QueryMode::from_flags (controller/mode.rs:231-247): web first
            if a.header:
                fh.write("tid\tidf\ttotal_match_count\tnode_count\tedge_count\tmax_node_cov\tmin_rmsd\tnres\tplddt\tmatching_residues\tdb_key\tquery_residues\n")
            query.sort_rows(rows, query.parse_sort_by(a.sort_by, True))   # StructureSortStrategy (sort.rs:400-458)
            for r in rows:
                fh.write(query.format_structure_row(r, r.get("query_residues", qstr)) + "\n")
        else:
            cols = [c.strip() for c in a.format_output.split(",") if c.strip()] or \
                (query.MATCH_SUPERPOSE_COLUMNS if (a.superpose or a.web) else ["tid", "node_count", "idf", "rmsd", "matching_residues", "query_residues"])
            for c in cols:
                if c not in query.MATCH_COLUMNS:
                    sys.exit(f"[FAIL] unknown --format-output column '{c}' (per-match: {', '.join(query.MATCH_COLUMNS)})")
            if a.header:
                fh.write("\t".join(cols) + "\n")
            for m in matches:
                fh.write(query.format_match_columns(m, cols) + "\n")
        if outp:
            fh.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="folddisco_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    pi = sub.add_parser("index")
    pi.add_argument("-p", "--pdbs", required=True)
    pi.add_argument("-i", "--index", default="")
    pi.add_argument("-t", "--threads", type=int, default=1)            # host threads of the structure ingest (the hashing and the posting build run on the GPU)
    pi.add_argument("-y", "--type", default="default")
    pi.add_argument("-d", "--distance", type=int, default=0)           # number of distance bins (0 -> 16), main.rs:38
    pi.add_argument("-a", "--angle", type=int, default=0)              # number of angle bins (0 -> 4)
    pi.add_argument("--multiple-bins", default=None)                   # d1-a1,d2-a2 e.g. 16-4,8-3 (build_index.rs:45)
    pi.add_argument("-g", "--grid", type=float, default=20.0)          # CA cutoff
    pi.add_argument("-n", "--residue", "--max-residue", dest="max_residue", type=int, default=50000)   # cli/main.rs:42: written to PREFIX.type only; the skip threshold is the reference's hard-wired 65535 (REF_SKIP_MAX_RESIDUE)
    pi.add_argument("-r", "--recursive", action="store_true")
    pi.add_argument("--id", default="relpath")                          # pdb | uniprot | afdb | relpath | abspath | basename ... (build_index.rs:40)
    pi.add_argument("-v", "--verbose", action="store_true")
    pi.add_argument("--device", type=int, default=0)
    pi.add_argument("--chunk", type=int, default=16384, help="structures per ingest step and GPU build call (the next chunk is parsed while this one is built; the sub-indices are merged on the device)")
    pi.add_argument("--coords", action="store_true", help="write PREFIX.coords, the coordinate store `query` reads instead of the structure files, in the same pass (single rank)")
    pi.add_argument("--mmap-on-disk", action="store_true", help="accepted for the reference's command lines (indextable.rs:215-226,247: there the posting array is filled in a file-backed "
                    "mapping of PREFIX instead of anonymous memory, the files are the same): here the array is filled in HBM and streamed to PREFIX either way")
    pq = sub.add_parser("query")
    pq.add_argument("-p", "--pdb", default="")
    pq.add_argument("-q", "--query", default="")
    pq.add_argument("-i", "--index", default="")
    pq.add_argument("-t", "--threads", type=int, default=1)
    pq.add_argument("-d", "--distance", default="0.5")
    pq.add_argument("-a", "--angle", default="5")
    pq.add_argument("--ca-distance", type=float, default=1.0)
    pq.add_argument("--top", type=int, default=None)
    pq.add_argument("--skip-match", action="store_true")
    pq.add_argument("--skip-ca-match", action="store_true")          # per-match rows before the C-alpha distance check (result.rs:54-69)
    pq.add_argument("--web", action="store_true")                    # per-match rows with superposition columns, at most 1000 lines (query_pdb.rs:142, 481-493)
    pq.add_argument("--partial-fit", action="store_true")            # LMS superposition for matches of > 3 residues (cli/main.rs:92)
    pq.add_argument("--per-structure", action="store_true")
    pq.add_argument("--per-match", action="store_true")
    pq.add_argument("--header", action="store_true")
    pq.add_argument("--serial-index", action="store_true")
    pq.add_argument("--freq-filter", type=float, default=None)
    pq.add_argument("--sampling-count", type=int, default=None)
    pq.add_argument("--sampling-ratio", type=float, default=None)
    pq.add_argument("--total-match", type=int, default=0)
    pq.add_argument("--covered-node", type=int, default=0)
    pq.add_argument("--covered-node-ratio", type=float, default=0.0)
    pq.add_argument("--max-node", type=int, default=0)
    pq.add_argument("--max-node-ratio", type=float, default=0.0)
    pq.add_argument("--score", type=float, default=0.0)
    pq.add_argument("--connected-node", type=int, default=0)
    pq.add_argument("--connected-node-ratio", type=float, default=0.0)
    pq.add_argument("--num-residue", type=int, default=50000)
    pq.add_argument("--plddt", type=float, default=0.0)
    pq.add_argument("--rmsd", type=float, default=0.0)
    pq.add_argument("--tm-score", type=float, default=0.0)
    pq.add_argument("--gdt-ts", type=float, default=0.0)
    pq.add_argument("--gdt-ha", type=float, default=0.0)
    pq.add_argument("--chamfer", type=float, default=0.0)
    pq.add_argument("--hausdorff", type=float, default=0.0)
    pq.add_argument("--format-output", default="")
    pq.add_argument("--superpose", action="store_true")              # print U, T and the matching C-alpha coordinates
    pq.add_argument("--sort-by", default="")          # cli/main.rs:84: empty -> MatchSortStrategy / StructureSortStrategy default (idf desc, rmsd asc)
    pq.add_argument("--length-penalty", type=float, default=None)
    pq.add_argument("-o", "--output", default="")
    pq.add_argument("-v", "--verbose", action="store_true")
    pq.add_argument("--device", type=int, default=0)
    pq.add_argument("--coords", default="", help="coordinate store to read the database's coordinates from (default: PREFIX.coords when it exists)")
    pq.add_argument("--no-coords", action="store_true", help="parse the structure files PREFIX.lookup names even when a coordinate store exists")
    pq.add_argument("--verify", action="store_true", help="check the loaded index first (see `verify`) and stop with status 1 if it is damaged")
    pu = sub.add_parser("update")                                    # index update without a rebuild (no counterpart in the reference)
    pu.add_argument("-i", "--index", required=True)
    pu.add_argument("-p", "--pdbs", default="", help="structures to append: a directory or a file, walked and ordered as `index` does")
    pu.add_argument("--remove", default="", help="text file with one tid per line (column 2 of PREFIX.lookup); every row with that tid is removed")
    pu.add_argument("-o", "--output", default="", help="output prefix (default: rewrite PREFIX in place)")
    pu.add_argument("--id", default="relpath", help="--id of the added structures' tids: the one the index was built with")
    pu.add_argument("-r", "--recursive", action="store_true")
    pu.add_argument("-t", "--threads", type=int, default=1)
    pu.add_argument("--chunk", type=int, default=16384)
    pu.add_argument("--device", type=int, default=0)
    pu.add_argument("-v", "--verbose", action="store_true")
    pu.add_argument("--verify", action="store_true", help="check the index before it is touched and the result before it is written (see `verify`); "
                    "status 1 and no file changed if either is damaged")
    pv = sub.add_parser("verify")                                    # is the index well formed? (no counterpart in the reference: it panics on use)
    pv.add_argument("-i", "--index", required=True)
    pv.add_argument("--host", action="store_true", help="decode on the CPU (no device is opened)")
    pv.add_argument("-t", "--threads", type=int, default=1, help="host threads of --host")
    pv.add_argument("--device", type=int, default=0)
    pv.add_argument("-v", "--verbose", action="store_true")
    pv.add_argument("--structures", action="store_true", help="also check that the index describes the coordinate store: every structure's row of the "
                    "index against the hashes of its coordinates (device only)")
    pv.add_argument("--coords", default="", help="coordinate store of --structures (default: PREFIX.coords)")
    pv.add_argument("--window", type=int, default=16384, help="structures compared per step of --structures")
    pw = sub.add_parser("rows")                                      # the hashes of chosen structures, read back from the index (no counterpart in the reference)
    pw.add_argument("-i", "--index", required=True, help="a single (unsharded) index prefix")
    pw.add_argument("-o", "--output", default="", help="the .npz file to write: hashes, row_off, ids, tids")
    pw.add_argument("--range", default=None, help="LO:HI, the structure ids LO .. HI - 1 (default: every structure)")
    pw.add_argument("--tids", default=None, help="text file with one tid per line (column 2 of PREFIX.lookup); the rows come out in the file's order")
    pw.add_argument("--window", type=int, default=16384, help="structures per walk over the index")
    pw.add_argument("--host", action="store_true", help="walk the index on the CPU (no device is opened)")
    pw.add_argument("-t", "--threads", type=int, default=1, help="host threads of --host")
    pw.add_argument("--device", type=int, default=0)
    pw.add_argument("--verify", action="store_true", help="check the loaded index first (see `verify`) and stop with status 1 if it is damaged")
    pw.add_argument("-v", "--verbose", action="store_true")
    pd = sub.add_parser("dups")                                      # which structures are already there? (no counterpart in the reference)
    pd.add_argument("-i", "--index", required=True, help="a single (unsharded) index prefix")
    pd.add_argument("--against", default=None, help="a second index prefix: every structure of PREFIX against every structure of it (default: inside PREFIX)")
    pd.add_argument("--min-similarity", type=float, default=0.9, help="report pairs whose sketches agree in at least this share of their filled buckets, in (0, 1]")
    pd.add_argument("--identical-only", action="store_true", help="only pairs with the same hash set (same size and digests)")
    pd.add_argument("--confirm", action="store_true", help="add the exact Jaccard similarity of every reported pair, from the rows of its structures")
    pd.add_argument("--min-jaccard", type=float, default=None, help="implies --confirm: keep only the reported pairs whose exact Jaccard similarity reaches this "
                    "floor, in (0, 1]")
    pd.add_argument("-o", "--output", default="", help="the TSV file to write (default: standard output)")
    pd.add_argument("--window", type=int, default=16384, help="structures per walk over the index")
    pd.add_argument("--max-pairs", type=int, default=1 << 24, help="most pairs to report; more end the command with their number")
    pd.add_argument("--host", action="store_true", help="reduce and compare on the CPU (no device is opened)")
    pd.add_argument("-t", "--threads", type=int, default=1, help="host threads of --host")
    pd.add_argument("--device", type=int, default=0)
    pd.add_argument("--verify", action="store_true", help="check every loaded index first (see `verify`) and stop with status 1 if it is damaged")
    pd.add_argument("-v", "--verbose", action="store_true")
    px = sub.add_parser("overlap")                                   # the exact similarity of given pairs, from their rows (no counterpart in the reference)
    px.add_argument("-i", "--index", required=True, help="a single (unsharded) index prefix")
    px.add_argument("--against", default=None, help="a second index prefix: tid_b of every pair is a structure of it (default: of PREFIX)")
    px.add_argument("--pairs", required=True, help="text file with one tid_a<TAB>tid_b per line (column 2 of the .lookup files); the rows come out in the file's order")
    px.add_argument("-o", "--output", default="", help="the TSV file to write (default: standard output)")
    px.add_argument("--min-jaccard", type=float, default=None, help="keep only the pairs whose exact Jaccard similarity reaches this floor, in (0, 1]")
    px.add_argument("--window", type=int, default=16384, help="structures per walk over the index")
    px.add_argument("--pool-mb", type=int, default=4096, help="megabytes of rows resident at a time, both sides of a tile together (4 bytes per hash)")
    px.add_argument("--host", action="store_true", help="extract and intersect on the CPU (no device is opened)")
    px.add_argument("-t", "--threads", type=int, default=1, help="host threads of --host")
    px.add_argument("--device", type=int, default=0)
    px.add_argument("--verify", action="store_true", help="check every loaded index first (see `verify`) and stop with status 1 if it is damaged")
    px.add_argument("-v", "--verbose", action="store_true")
    px.set_defaults(max_pairs=0, min_similarity=1.0)                 # what the shared planning of `dups` looks at
    pn = sub.add_parser("neighbors")                               # the k nearest structures of every structure, by signature (no counterpart in the reference)
    pn.add_argument("-i", "--index", required=True, help="a single (unsharded) index prefix")
    pn.add_argument("--against", default=None, help="a second index prefix: the neighbours are looked for among its structures (default: among the others of PREFIX)")
    pn.add_argument("-k", type=int, default=8, help="neighbours per structure, 1..32")
    pn.add_argument("--min-similarity", type=float, default=None, help="the share of agreeing filled buckets a neighbour must reach, in (0, 1] (default: 1 / 64)")
    pn.add_argument("--exact", action="store_true", help="the k nearest by the exact Jaccard similarity of the rows, counted from the posting lists, instead of by signature")
    pn.add_argument("--min-jaccard", type=float, default=None, help="with --exact: the exact Jaccard similarity a neighbour must reach, in (0, 1] (default: any shared hash)")
    pn.add_argument("--pool-mb", type=int, default=4096, help="megabytes of rows resident at a time (4 bytes per hash)")
    pn.add_argument("--counter-mb", type=int, default=1024, help="with --exact: megabytes of the counter table (4 bytes per query of a block and structure)")
    pn.add_argument("--tids", default=None, help="text file with one tid per line (column 2 of PREFIX.lookup): only these structures are queries")
    pn.add_argument("--confirm", action="store_true", help="add the exact Jaccard similarity of every row, from the rows of its structures")
    pn.add_argument("-o", "--output", default="", help="the TSV file to write (default: standard output)")
    pn.add_argument("--window", type=int, default=16384, help="structures per walk over the index")
    pn.add_argument("--host", action="store_true", help="reduce and select on the CPU (no device is opened)")
    pn.add_argument("-t", "--threads", type=int, default=1, help="host threads of --host")
    pn.add_argument("--device", type=int, default=0)
    pn.add_argument("--verify", action="store_true", help="check every loaded index first (see `verify`) and stop with status 1 if it is damaged")
    pn.add_argument("-v", "--verbose", action="store_true")
    pk = sub.add_parser("cluster")                                   # one representative per group of similar structures, by signature (no counterpart in the reference)
    pk.add_argument("-i", "--index", required=True, help="a single (unsharded) index prefix")
    pk.add_argument("--against", default=None, help="a second index prefix whose structures are representatives from the start: which structures of PREFIX are new?")
    pk.add_argument("--against-reps", default=None, help="text file with one tid per line (column 2 of PREFIX2.lookup): only these structures of --against are seeds")
    pk.add_argument("--representatives", default="", help="also write the (new) representatives' tids, one per line: appended to the seeds' list, the next --against-reps")
    pk.add_argument("--min-similarity", type=float, default=0.9, help="a structure joins a representative whose sketch agrees with its own in at least this share of their filled buckets, in (0, 1]")
    pk.add_argument("--rep-by", default="hashes", help="the walk order, earlier structures represent: hashes (the row's size, descending; default), nres or plddt "
                    "(that column of PREFIX.lookup, descending), id (ascending); ties by id")
    pk.add_argument("-o", "--output", default="", help="the TSV file to write (default: standard output)")
    pk.add_argument("--redundant", default="", help="also write the members' tids, one per line: the file `update --remove` takes")
    pk.add_argument("--confirm", action="store_true", help="add the exact Jaccard similarity of every member with its representative, from their rows")
    pk.add_argument("--min-jaccard", type=float, default=None, help="implies --confirm: --redundant lists only the members whose exact Jaccard similarity with "
                    "their representative reaches this floor, in (0, 1]; a member below it is kept")
    pk.add_argument("--window", type=int, default=16384, help="structures per walk over the index")
    pk.add_argument("--host", action="store_true", help="reduce and cluster on the CPU (no device is opened)")
    pk.add_argument("-t", "--threads", type=int, default=1, help="host threads of --host")
    pk.add_argument("--device", type=int, default=0)
    pk.add_argument("--verify", action="store_true", help="check the loaded index first (see `verify`) and stop with status 1 if it is damaged")
    pk.add_argument("-v", "--verbose", action="store_true")
    pr = sub.add_parser("reshard")                                   # one index <-> shards by structure id range (no counterpart in the reference)
    pr.add_argument("-i", "--index", required=True)
    pr.add_argument("--to", type=int, required=True, help="shards to write (PREFIX.shard<r>ofW); 1 writes the single index")
    pr.add_argument("--from", dest="from_", type=int, default=1, help="shards to read (PREFIX.shard<k>ofV); 1 (default) reads the single index")
    pr.add_argument("-o", "--output", default="", help="output prefix (default: beside PREFIX); .lookup and .type are copied to it")
    pr.add_argument("--host", action="store_true", help="merge and cut on the CPU (no device is opened)")
    pr.add_argument("-t", "--threads", type=int, default=1, help="host threads of --host")
    pr.add_argument("--device", type=int, default=0)
    pr.add_argument("--verify", action="store_true", help="check what was loaded and every part, each with its own id range, before anything is written (see `verify`)")
    pr.add_argument("-v", "--verbose", action="store_true")
    pm = sub.add_parser("merge")                                     # indices built separately -> one index (no counterpart in the reference)
    pm.add_argument("-i", "--index", nargs="+", required=True, help="2 to 64 single (unsharded) index prefixes, joined in the order given")
    pm.add_argument("-o", "--output", default="", help="output prefix (required, none of the inputs)")
    pm.add_argument("--host", action="store_true", help="rebase and merge on the CPU (no device is opened)")
    pm.add_argument("-t", "--threads", type=int, default=1, help="host threads of --host")
    pm.add_argument("--device", type=int, default=0)
    pm.add_argument("--verify", action="store_true", help="check every loaded input and the joined index before anything is written (see `verify`)")
    pm.add_argument("-v", "--verbose", action="store_true")
    po = sub.add_parser("reorder")                                   # the index's structures in another order (no counterpart in the reference)
    po.add_argument("-i", "--index", required=True, help="a single (unsharded) index prefix")
    po.add_argument("--by", default=None, help="sort PREFIX.lookup by one column: tid (byte string), nres or plddt (numeric); stable")
    po.add_argument("--order", default=None, help="text file with one tid per line: the new order; it must name every tid of PREFIX.lookup exactly once")
    po.add_argument("--desc", action="store_true", help="--by in descending order (ties keep their old order)")
    po.add_argument("-o", "--output", default="", help="output prefix (default: rewrite PREFIX in place)")
    po.add_argument("--host", action="store_true", help="reorder on the CPU (no device is opened)")
    po.add_argument("-t", "--threads", type=int, default=1, help="host threads of --host")
    po.add_argument("--device", type=int, default=0)
    po.add_argument("--verify", action="store_true", help="check the loaded index and the result before anything is written (see `verify`)")
    po.add_argument("-v", "--verbose", action="store_true")
    pc = sub.add_parser("coords")                                    # the coordinate store of an existing index (no counterpart in the reference)
    pc.add_argument("-i", "--index", required=True)
    pc.add_argument("-o", "--output", default="", help="file to write (default: PREFIX.coords)")
    pc.add_argument("-t", "--threads", type=int, default=1, help="host threads of the structure ingest")
    pc.add_argument("--chunk", type=int, default=16384, help="structures parsed per step")
    pc.add_argument("-v", "--verbose", action="store_true")
    pa = sub.add_parser("analyze")                                   # src/cli/workflows/analyze.rs:19-40 (summary branch)
    pa.add_argument("-i", "--index", required=True)
    pa.add_argument("-p", "--pdbs", default=None)
    pa.add_argument("-o", "--output", default=None)
    pa.add_argument("--top", type=int, default=10)
    pa.add_argument("--p-value", type=float, default=0.0001)
    pa.add_argument("--min-support", type=int, default=4)
    pa.add_argument("--max-pos", type=int, default=32)
    pa.add_argument("-t", "--threads", type=int, default=1)
    pa.add_argument("-v", "--verbose", action="store_true")
    pa.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.cmd == "analyze":
        from folddisco_amd import analyze
        if a.pdbs is not None:                                       # enrichment branch (analyze.rs:111-132)
            import folddisco_amd as fd
            paths = _load_paths(a.pdbs, False)
            if not paths:
                sys.exit(f"[FAIL] no structures under {a.pdbs}")
            out = a.output or f"{a.pdbs}_vs_{a.index.split('/')[-1]}"    # analyze.rs:74-79
            ctx = fd.Context(getattr(a, "device", 0))
            en = analyze.enrichment(ctx, a.index, paths, a.p_value, a.threads)
            analyze.save_enrichment(en, paths, out, a.min_support, a.max_pos)
            return
        out = a.output or f"{a.index}_summary"                       # analyze.rs:71-84
        analyze.save_summary(analyze.summarize(a.index), out, a.top)
        return
    if a.cmd == "update":
        cmd_update(a)
        return
    if a.cmd == "verify":
        cmd_verify(a)
        return
    if a.cmd == "rows":
        cmd_rows(a)
        return
    if a.cmd == "dups":
        cmd_dups(a)
        return
    if a.cmd == "overlap":
        cmd_overlap(a)
        return
    if a.cmd == "neighbors":
        cmd_neighbors(a)
        return
    if a.cmd == "cluster":
        cmd_cluster(a)
        return
    if a.cmd == "reshard":
        cmd_reshard(a)
        return
    if a.cmd == "merge":
        cmd_merge(a)
        return
    if a.cmd == "reorder":
        cmd_reorder(a)
        return
    if a.cmd == "coords":
        cmd_coords(a)
        return
    if a.cmd == "index":
        if a.mmap_on_disk and a.verbose:
            # the reference's switch chooses WHERE the posting array lives while it is filled (a mapping of PREFIX on disk, indextable.rs:215-226, or
            # anonymous memory copied to PREFIX afterwards, :247-270); PREFIX, PREFIX.offset, .lookup and .type are byte for byte the same in both modes
            print("[INFO] --mmap-on-disk: the posting array is filled in HBM and streamed to PREFIX (same files as without the flag)", file=sys.stderr)
        try:
            a.hash_type = hash_type_index(a.type)
        except ValueError:
            sys.exit(f"[FAIL] unknown hash type {a.type}")
        a.multi = parse_multiple_bins(a.multiple_bins) if a.multiple_bins else None
        if a.multi is not None and a.hash_type in (2, 4, 5, 6):
            sys.exit("[FAIL] --multiple-bins is implemented for the encodings over the PDBTrRosetta descriptor only")
        if a.multi is not None and (not a.multi or len(a.multi) > 8 or any(d == 0 or x == 0 for d, x in a.multi)):
            sys.exit("[FAIL] --multiple-bins: one to eight dist-angle pairs with non-zero counts, e.g. 16-4,8-3")
        cmd_index(a)
    else:
        if a.per_structure and a.per_match:
            sys.exit("[FAIL] --per-structure and --per-match cannot be combined")     # ContradictoryPrintError
        cmd_query(a)


if __name__ == "__main__":
    main()
