"""On-disk index files: PREFIX (value bytes), PREFIX.offset, PREFIX.lookup, PREFIX.type.

The two binary files are written by libfdgpu (`fdgpu_index_save`) or by `write_index_files` for a merged index;
`.lookup` (src/index/lookup.rs:35-56) and `.type` (src/cli/config.rs:66-97) are small text files written here."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import u8p, u32p, u64p


def format_f32_display(v) -> str:
    """Rust `{}` for f32: shortest digits that round-trip, never exponent form, integral values without fraction."""
    v = np.float32(v)
    if np.isnan(v):
        return "NaN"
    if np.isinf(v):
        return "inf" if v > 0 else "-inf"
    for prec in range(1, 10):
        s = "%.*e" % (prec - 1, float(v))
        if np.float32(float(s)) == v:
            break
    mant, ex = s.split("e")
    neg = mant.startswith("-")
    digits = mant.lstrip("-").replace(".", "").rstrip("0") or "0"
    ex = int(ex)
    if ex < 0:
        out = "0." + "0" * (-ex - 1) + digits
    elif len(digits) <= ex + 1:
        out = digits + "0" * (ex + 1 - len(digits))
    else:
        out = digits[: ex + 1] + "." + digits[ex + 1:]
    return ("-" if neg else "") + out          # -0.0 -> "-0" like Rust


_ID_TYPES = {"Pdb": "pdb", "PDB": "pdb", "pdb": "pdb", "Afdb": "afdb", "AFDB": "afdb", "afdb": "afdb", "Uniprot": "uniprot", "UniProt": "uniprot",
             "uniprot": "uniprot", "BasenameWithoutExt": "stem", "basename_without_ext": "stem", "basename_no_ext": "stem", "filename": "stem",
             "BasenameWithExt": "name", "basename_with_ext": "name", "basename": "name", "file": "name", "AbsPath": "abs", "Abspath": "abs",
             "abspath": "abs", "absolute_path": "abs", "path": "abs", "RelPath": "rel", "Relpath": "rel", "relpath": "rel", "relative_path": "rel",
             "default": "rel"}


def parse_path_by_id_type(path: str, id_type: str) -> str:
    """--id of the index subcommand: IdType::get_with_str + parse_path_by_id_type (src/controller/mode.rs:18-30, 69-126).
    file_stem drops only the last extension (x.pdb.gz -> x.pdb), like std::path::Path::file_stem."""
    import re
    kind = _ID_TYPES.get(id_type, "other")
    name = os.path.basename(path.rstrip("/")) if kind != "abs" else ""
    stem = name[: name.rfind(".")] if name.rfind(".") > 0 else name
    if kind == "pdb":
        return stem[3:] if stem.startswith("pdb") else stem
    if kind in ("afdb", "uniprot"):
        m = re.search(r"AF-.+-model_v\d", stem)
        if not m:
            return stem
        return m.group(0) if kind == "afdb" else m.group(0).split("-")[1]
    if kind == "stem":
        return stem
    if kind == "name":
        return name
    if kind == "abs":
        return os.path.realpath(path)
    return path


def save_lookup(path: str, tids, nres, plddt, db_keys=None):
    """PREFIX.lookup through the library's writer (fdgpu_write_lookup: 20,500 lines cost 0.1 s of Python float formatting otherwise).  An id with a
    newline inside (no path has one) takes the Python writer, which is also what the tests compare the library's bytes with."""
    tids = [str(t) for t in tids]
    n = len(tids)
    if any("\n" in t for t in tids):
        return save_lookup_py(path, tids, nres, plddt, db_keys)
    nr = np.ascontiguousarray(nres, dtype=np.uint64)
    pl = np.ascontiguousarray(plddt, dtype=np.float32)
    dk = None if db_keys is None else np.ascontiguousarray(db_keys, dtype=np.uint64)
    assert len(nr) >= n and len(pl) >= n and (dk is None or len(dk) >= n)
    rc = _lib.load().fdgpu_write_lookup(os.fsencode(path), "\n".join(tids).encode(), n, nr.ctypes.data_as(u64p), pl.ctypes.data_as(_lib.f32p),
                                        None if dk is None else dk.ctypes.data_as(u64p))
    if rc != 0:
        raise IOError(f"cannot write {path}")


def save_lookup_py(path: str, tids, nres, plddt, db_keys=None):
    with open(path, "w") as f:
        for i, tid in enumerate(tids):
            f.write(f"{i}\t{tid}\t{int(nres[i])}\t{format_f32_display(plddt[i])}\t{i if db_keys is None else int(db_keys[i])}\n")


def load_lookup(path: str):
    tids, nres, plddt, keys = [], [], [], []
    with open(path) as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            tids.append(p[1]); nres.append(int(p[2])); plddt.append(np.float32(p[3])); keys.append(int(p[4]) if len(p) > 4 else int(p[0]))
    return tids, np.array(nres, np.uint64), np.array(plddt, np.float32), np.array(keys, np.uint64)


def read_lookup_rows(path: str):
    """PREFIX.lookup as its raw lines (newline kept), for the index update's verbatim rewrite"""
    with open(path, newline="") as f:
        return f.readlines()


def update_lookup_rows(rows, keep, keep_db_keys: bool):
    """the kept rows of PREFIX.lookup after an index update: tid, nres and plddt verbatim, the id renumbered densely in the old order; the
    db_key column renumbered too for a file-built index (there it equals the id) and left as it was for a Foldcomp-built one (its database key)"""
    keep = np.asarray(keep, dtype=bool)
    if len(keep) != len(rows):
        raise ValueError(f"keep: {len(rows)} entries expected, got {len(keep)}")
    out, i = [], 0
    for row, k in zip(rows, keep):
        if not k:
            continue
        p = row.rstrip("\n").split("\t")
        p[0] = str(i)
        if len(p) > 4 and not keep_db_keys:
            p[4] = str(i)
        out.append("\t".join(p) + "\n")
        i += 1
    return out


def lookup_rows(first: int, tids, nres, plddt, db_keys=None):
    """PREFIX.lookup lines of structures first, first + 1, ... (the format of save_lookup)"""
    return [f"{first + i}\t{tid}\t{int(nres[i])}\t{format_f32_display(plddt[i])}\t{first + i if db_keys is None else int(db_keys[i])}\n"
            for i, tid in enumerate(tids)]


def update_type_text(text: str, n_structures: int) -> str:
    """PREFIX.type after an index update: chunk_size = the new number of structures, every other line as it was"""
    lines = text.splitlines(keepends=True)
    hit = [k for k, line in enumerate(lines) if line.split("=", 1)[0].strip() == "chunk_size"]
    if len(hit) != 1:
        raise ValueError("index type file: no chunk_size line")
    lines[hit[0]] = f"chunk_size = {int(n_structures)}\n"
    return "".join(lines)


def save_type(path: str, n_structures: int, grid_width: float = 20.0, max_residue: int = 50000, nbin_angle: int = 0, nbin_dist: int = 0,
              input_format: str = "PDB", hash_type: str = "PDBTrRosetta", multiple_bins=None, foldcomp_db=None):
    """IndexConfig::to_toml (cli/config.rs:66-87): keys in alphabetical order (toml's table is a BTreeMap)"""
    gw = repr(float(grid_width))  # toml prints the f64; 20.0 -> "20.0"
    with open(path, "w") as f:
        f.write(f"chunk_size = {n_structures}\n" + (f"foldcomp_db = \"{foldcomp_db}\"\n" if foldcomp_db else "") + f"grid_width = {gw}\nhash_type = \"{hash_type}\"\ninput_format = \"{input_format}\"\n"
                f"max_residue = {max_residue}\n" + (("multiple_bin = [" + ", ".join(f"[{d}, {a}]" for d, a in multiple_bins) + "]\n") if multiple_bins else "") +
                f"num_bin_angle = {nbin_angle}\nnum_bin_dist = {nbin_dist}\n")


def load_type(path: str) -> dict:
    out = {}
    for line in open(path):
        if "=" in line:
            k, v = (t.strip() for t in line.split("=", 1))
            if v.startswith("[["):    # multiple_bin = [[16, 4], [8, 3]] (cli/config.rs:48-53, 78-84)
                out[k] = [tuple(int(x) for x in item.split(",")) for item in v.strip()[2:-2].split("], [")]
            else:
                out[k] = v.strip('"') if v.startswith('"') else (float(v) if "." in v else int(v))
    return out


def write_index_files(prefix: str, value: np.ndarray, hashes: np.ndarray, offsets: np.ndarray):
    """PREFIX and PREFIX.offset (u64 H | u32 hashes[H] | u64 offsets[H+1]), src/index/indextable.rs:297-326"""
    np.ascontiguousarray(value, np.uint8).tofile(prefix)
    with open(prefix + ".offset", "wb") as f:
        f.write(np.uint64(len(hashes)).tobytes())
        f.write(np.ascontiguousarray(hashes, np.uint32).tobytes())
        f.write(np.ascontiguousarray(offsets, np.uint64).tobytes())


def read_index_files(prefix: str):
    """-> (value, hashes, offsets); accepts the legacy PREFIX.value name (indextable.rs:333-337)"""
    vp = prefix + ".value" if os.path.exists(prefix + ".value") else prefix
    value = np.fromfile(vp, dtype=np.uint8)
    raw = np.fromfile(prefix + ".offset", dtype=np.uint8)
    H = int(raw[:8].view(np.uint64)[0])
    if len(raw) < 8 + 4 * H + 8 * (H + 1):
        raise ValueError("offset file is in an old format or corrupted")
    hashes = raw[8: 8 + 4 * H].view(np.uint32).copy()
    offsets = raw[8 + 4 * H: 8 + 4 * H + 8 * (H + 1)].copy().view(np.uint64)
    return value, hashes, offsets


VERIFY_CLASSES = ("OFFSET_ENDS", "OFFSET_ORDER", "HASH_ORDER", "LIST_END", "VARINT_LONG", "VARINT_FORM", "ZERO_DELTA", "ID_RANGE")      # classes 1..8 (csrc/fd_verify.h)


@dataclass
class VerifyReport:
    """fd_verify_report: the verdict of FolddiscoIndex.verify / verify_host.  counts: slots per class name; first_*: the lowest bad slot (None when ok);
    the totals are those of a clean index (0 otherwise)."""
    ok: bool
    n_bad: int
    counts: dict
    first_slot: int | None
    first_hash: int | None
    first_offset: int | None
    first_classes: tuple
    list_stage: bool
    n_lists: int
    n_postings: int
    max_id: int
    max_list_bytes: int

    @staticmethod
    def from_c(r) -> "VerifyReport":
        ok = bool(r.ok)
        return VerifyReport(ok=ok, n_bad=int(r.n_bad), counts={n: int(r.class_count[c + 1]) for c, n in enumerate(VERIFY_CLASSES)},
                            first_slot=None if ok else int(r.first_slot), first_hash=None if ok else int(r.first_hash),
                            first_offset=None if ok else int(r.first_offset),
                            first_classes=tuple(n for c, n in enumerate(VERIFY_CLASSES) if r.first_mask >> c & 1), list_stage=bool(r.list_stage),
                            n_lists=int(r.n_lists), n_postings=int(r.n_postings), max_id=int(r.max_id), max_list_bytes=int(r.max_list_bytes))

    def __str__(self) -> str:
        if self.ok:
            return f"[OK] index is well formed: {self.n_lists} lists, {self.n_postings} postings, max id {self.max_id}, longest list {self.max_list_bytes} bytes"
        counts = ", ".join(f"{n} {v}" for n, v in self.counts.items() if v)
        return (f"[FAIL] index is damaged: {self.n_bad} bad slot(s); first at slot {self.first_slot} (hash {self.first_hash}, offset {self.first_offset}): "
                f"{'+'.join(self.first_classes)}; slots per class: {counts}")


def verify_host(value, hashes, offsets, n_structures: int, first_id: int = 0, threads: int = 1) -> VerifyReport:
    """the index checks of csrc/fd_verify.h on host arrays (fdgpu_verify_host): no context, no device"""
    value = np.ascontiguousarray(value, dtype=np.uint8)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) != len(hashes) + 1:
        raise ValueError(f"offsets: {len(hashes) + 1} entries expected, got {len(offsets)}")
    r = _lib.VerifyReportC()
    rc = _lib.load().fdgpu_verify_host(hashes.ctypes.data_as(u32p), offsets.ctypes.data_as(u64p), len(hashes), value.ctypes.data_as(u8p), len(value),
                                       int(first_id), int(n_structures), max(int(threads), 1), C.byref(r))
    if rc != 0:
        raise ValueError(f"fdgpu_verify_host failed ({rc})")
    return VerifyReport.from_c(r)


def check_value_offset_pair(prefix: str) -> list:
    """PREFIX and PREFIX.offset (both present) against each other without decoding a posting: the offset file's header against its own size, its
    last offset against the value file's size -> a list of complaints"""
    bad = []
    osz, vsz = os.path.getsize(prefix + ".offset"), os.path.getsize(prefix)
    if osz < 16:
        bad.append(f"{prefix}.offset: {osz} bytes, shorter than an empty table (16)")
    else:
        with open(prefix + ".offset", "rb") as f:
            H = int(np.frombuffer(f.read(8), np.uint64)[0])
            want = 8 + 4 * H + 8 * (H + 1)
            if osz != want:
                bad.append(f"{prefix}.offset: {osz} bytes, its header ({H} hashes) asks for {want}")
            else:
                f.seek(want - 8)
                end = int(np.frombuffer(f.read(8), np.uint64)[0])
                if end != vsz:
                    bad.append(f"{prefix}: {vsz} bytes, the last offset of {prefix}.offset is {end}")
    return bad


def check_lookup_type(prefix: str):
    """PREFIX.lookup and PREFIX.type (both present): row k starts with id k, chunk_size equals the rows -> (complaints, rows)"""
    bad = []
    n_rows, rows_ok = 0, True
    with open(prefix + ".lookup") as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            if rows_ok and (len(p) < 4 or p[0] != str(n_rows)):
                bad.append(f"{prefix}.lookup: row {n_rows + 1} does not start with id {n_rows} (or has fewer than four columns)")
                rows_ok = False
            n_rows += 1
    try:
        cs = load_type(prefix + ".type").get("chunk_size")
    except (ValueError, IndexError) as e:
        cs = None
        bad.append(f"{prefix}.type does not parse: {e}")
    else:
        if not isinstance(cs, int):
            bad.append(f"{prefix}.type: no integer chunk_size")
        elif cs != n_rows:
            bad.append(f"{prefix}.type: chunk_size = {cs}, {prefix}.lookup has {n_rows} rows")
    return bad, n_rows


def check_index_files(prefix: str) -> list:
    """what can be said about an index's four files without decoding a posting: -> a list of complaints, empty if there is none.
    chunk_size of PREFIX.type must equal the rows of PREFIX.lookup: `index` and `update` write it so, and so does the reference
    (build_index.rs:133, 218: the number of input paths, one .lookup row each)."""
    bad = []
    for ext in ("", ".offset", ".lookup", ".type"):
        if not os.path.isfile(prefix + ext):
            bad.append(f"{prefix}{ext} not found")
    if bad:
        return bad
    return check_value_offset_pair(prefix) + check_lookup_type(prefix)[0]


def merge_subindices(parts):
    """parts: list of (value u8[], hashes u32[], offsets u64[]) over ascending id ranges -> merged (value, hashes, offsets)"""
    L = _lib.load()
    n = len(parts)
    vals = [np.ascontiguousarray(p[0], np.uint8) for p in parts]
    hs = [np.ascontiguousarray(p[1], np.uint32) for p in parts]
    offs = [np.ascontiguousarray(p[2], np.uint64) for p in parts]
    vp = (u8p * n)(*[v.ctypes.data_as(u8p) for v in vals])
    hp = (u32p * n)(*[h.ctypes.data_as(u32p) for h in hs])
    op = (u64p * n)(*[o.ctypes.data_as(u64p) for o in offs])
    nh = np.array([len(h) for h in hs], np.uint64)
    ov, oh, oo = u8p(), u32p(), u64p()
    vl, H = C.c_uint64(), C.c_uint64()
    rc = L.fdgpu_merge_subindices(n, vp, hp, op, nh.ctypes.data_as(u64p), C.byref(ov), C.byref(vl), C.byref(oh), C.byref(oo), C.byref(H))
    if rc != 0:
        raise RuntimeError(f"fdgpu_merge_subindices failed ({rc}): parts must cover ascending id ranges")
    v = np.ctypeslib.as_array(ov, shape=(max(vl.value, 1),))[: vl.value].copy()
    h = np.ctypeslib.as_array(oh, shape=(max(H.value, 1),))[: H.value].copy()
    o = np.ctypeslib.as_array(oo, shape=(H.value + 1,)).copy()
    for p in (ov, oh, oo):
        L.fdgpu_free(p)
    return v, h, o


def shard_range(rank: int, world: int, n_structures: int):
    """contiguous, balanced id ranges; the union over ranks is [0, n_structures)"""
    base, rem = divmod(n_structures, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_bounds(world: int, n_structures: int) -> np.ndarray:
    """the world + 1 cut points of shard_range: shard r of a sharded build or a `reshard` holds the ids [bounds[r], bounds[r + 1])"""
    return np.array([shard_range(r, world, n_structures)[0] for r in range(world)] + [n_structures], dtype=np.uint64)


def split_host(value, hashes, offsets, bounds, first_id: int = 0, threads: int = 1):
    """the cut of an index by structure id range on host arrays (fdgpu_split_host: no context, no device), the inverse of merge_subindices:
    -> list of (value, hashes, offsets), part r with the ids in [bounds[r], bounds[r + 1]) unchanged"""
    value = np.ascontiguousarray(value, dtype=np.uint8)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) != len(hashes) + 1:
        raise ValueError(f"offsets: {len(hashes) + 1} entries expected, got {len(offsets)}")
    b = np.ascontiguousarray(bounds, dtype=np.uint64)
    n = len(b) - 1
    if b.ndim != 1 or n < 0:
        raise ValueError("bounds: a 1-d array of n_parts + 1 ids expected")
    L = _lib.load()
    ov, oh, oo = (u8p * max(n, 1))(), (u32p * max(n, 1))(), (u64p * max(n, 1))()
    vl, nh = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
    rc = L.fdgpu_split_host(hashes.ctypes.data_as(u32p), offsets.ctypes.data_as(u64p), len(hashes), value.ctypes.data_as(u8p), len(value), int(first_id),
                            n, b.ctypes.data_as(u64p), max(int(threads), 1), ov, vl.ctypes.data_as(u64p), oh, oo, nh.ctypes.data_as(u64p))
    if rc != 0:
        raise ValueError(f"fdgpu_split_host failed ({rc}): bounds must ascend from first_id (1 to 64 parts) and cover every id of the index")
    parts = []
    for r in range(n):
        V, H = int(vl[r]), int(nh[r])
        parts.append((np.ctypeslib.as_array(ov[r], shape=(max(V, 1),))[:V].copy(), np.ctypeslib.as_array(oh[r], shape=(max(H, 1),))[:H].copy(),
                      np.ctypeslib.as_array(oo[r], shape=(H + 1,)).copy()))
        for p in (ov[r], oh[r], oo[r]):
            L.fdgpu_free(p)
    return parts


def rebase_host(value, hashes, offsets, first_id: int, new_first_id: int, n_structures: int, threads: int = 1):
    """an index moved to the ids new_first_id .. new_first_id + n_structures - 1 on host arrays (fdgpu_rebase_host: no context, no device):
    -> (value, hashes, offsets), what a build over the same structures with first_id = new_first_id gives.  Raises ValueError with the library's
    code in it: -4 (FDGPU_ERANGE) for ids beyond 32 bits or a list of 4 GiB, -1 (FDGPU_EINVAL) for a damaged index"""
    value = np.ascontiguousarray(value, dtype=np.uint8)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) != len(hashes) + 1:
        raise ValueError(f"offsets: {len(hashes) + 1} entries expected, got {len(offsets)}")
    L = _lib.load()
    ov, oh, oo = u8p(), u32p(), u64p()
    vl = C.c_uint64()
    rc = L.fdgpu_rebase_host(hashes.ctypes.data_as(u32p), offsets.ctypes.data_as(u64p), len(hashes), value.ctypes.data_as(u8p), len(value), int(first_id),
                             int(new_first_id), int(n_structures), max(int(threads), 1), C.byref(ov), C.byref(vl), C.byref(oh), C.byref(oo))
    if rc != 0:
        raise ValueError(f"fdgpu_rebase_host failed ({rc}): " + ("the new id range or a list exceeds 32 bits" if rc == -4 else
                         "the index is damaged or holds first ids outside [first_id, first_id + n_structures)"))
    H = len(hashes)
    v = np.ctypeslib.as_array(ov, shape=(max(vl.value, 1),))[: vl.value].copy()
    h = np.ctypeslib.as_array(oh, shape=(max(H, 1),))[:H].copy()
    o = np.ctypeslib.as_array(oo, shape=(H + 1,)).copy()
    for p in (ov, oh, oo):
        L.fdgpu_free(p)
    return v, h, o


def permute_host(value, hashes, offsets, new_id, first_id: int = 0, threads: int = 1):
    """an index with its structures in another order on host arrays (fdgpu_permute_host: no context, no device): new_id[k] = new local position of
    the structure now at local position k, a permutation of 0 .. n - 1 -> (value, hashes, offsets), what a build over the same structures taken in
    the new order gives.  Raises ValueError with the library's code in it: -1 (FDGPU_EINVAL) for a new_id that is no permutation, an id outside
    [first_id, first_id + n) or a damaged index, -4 (FDGPU_ERANGE) for a list of 4 GiB"""
    value = np.ascontiguousarray(value, dtype=np.uint8)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) != len(hashes) + 1:
        raise ValueError(f"offsets: {len(hashes) + 1} entries expected, got {len(offsets)}")
    p = np.asarray(new_id)
    if p.ndim != 1 or (len(p) and (p.dtype.kind not in "iu" or p.min() < 0 or p.max() > 0xffffffff)):
        raise ValueError("fdgpu_permute_host failed (-1): new_id must be a 1-d array of positions 0 .. n - 1")
    p = np.ascontiguousarray(p, dtype=np.uint32)
    L = _lib.load()
    ov, oh, oo = u8p(), u32p(), u64p()
    vl = C.c_uint64()
    rc = L.fdgpu_permute_host(hashes.ctypes.data_as(u32p), offsets.ctypes.data_as(u64p), len(hashes), value.ctypes.data_as(u8p), len(value), int(first_id),
                              p.ctypes.data_as(u32p), len(p), max(int(threads), 1), C.byref(ov), C.byref(vl), C.byref(oh), C.byref(oo))
    if rc != 0:
        raise ValueError(f"fdgpu_permute_host failed ({rc}): " + ("a list exceeds 32 bits" if rc == -4 else
                         "new_id is not a permutation of 0 .. n - 1, or the index is damaged or holds ids outside [first_id, first_id + n)"))
    H = len(hashes)
    v = np.ctypeslib.as_array(ov, shape=(max(vl.value, 1),))[: vl.value].copy()
    h = np.ctypeslib.as_array(oh, shape=(max(H, 1),))[:H].copy()
    o = np.ctypeslib.as_array(oo, shape=(H + 1,)).copy()
    for q in (ov, oh, oo):
        L.fdgpu_free(q)
    return v, h, o


def rows_host(value, hashes, offsets, n_structures: int, first_id: int = 0, lo=None, hi=None, threads: int = 1):
    """rows of the transposed index from host arrays (fdgpu_rows_host: no context, no device): for the structures lo .. hi - 1 (absolute ids;
    default: the whole index) -> (hashes u32[...], row_off u64[hi - lo + 1]), hashes[row_off[k]: row_off[k + 1]] = the ascending hashes whose
    posting lists hold structure lo + k.  The result does not depend on `threads`.  Raises ValueError with the library's code in it: -1
    (FDGPU_EINVAL) for a window outside the index or a damaged index, -4 (FDGPU_ERANGE) for a list of 4 GiB or 2^32 postings in the window"""
    value = np.ascontiguousarray(value, dtype=np.uint8)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) != len(hashes) + 1:
        raise ValueError(f"offsets: {len(hashes) + 1} entries expected, got {len(offsets)}")
    lo = int(first_id) if lo is None else int(lo)
    hi = int(first_id) + int(n_structures) if hi is None else int(hi)
    if lo < 0 or hi < lo:
        raise ValueError("fdgpu_rows_host failed (-1): lo <= hi, absolute structure ids, expected")
    L = _lib.load()
    oh, oo = u32p(), u64p()
    rc = L.fdgpu_rows_host(hashes.ctypes.data_as(u32p), offsets.ctypes.data_as(u64p), len(hashes), value.ctypes.data_as(u8p), len(value), int(first_id),
                           int(n_structures), lo, hi, max(int(threads), 1), C.byref(oh), C.byref(oo))
    if rc != 0:
        raise ValueError(f"fdgpu_rows_host failed ({rc}): " + ("a list reaches 4 GiB or the window holds 2^32 postings" if rc == -4 else
                         "the window is not inside the index, or the index is damaged or holds ids outside [first_id, first_id + n_structures)"))
    off = _lib.owned_view(L, oo, (hi - lo + 1) * 8, np.uint64)
    return _lib.owned_view(L, oh, int(off[-1]) * 4, np.uint32), off


# ---- exact row overlaps (include/fdgpu.h: fdgpu_rowset, fdgpu_rows_intersect_host) ------------------------------------------------------------
# For structures a and b with rows R_a, R_b: inter = |R_a ∩ R_b|, union = |R_a| + |R_b| - inter, jaccard = inter / max(union, 1).  Integers only.
OVERLAP_POOL_HASHES = 1 << 30      # 4096 MB of u32 hashes, both sides of a tile together


def _csr_rows(rows, name):
    h, off = rows
    h = np.ascontiguousarray(h, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    if h.ndim != 1 or off.ndim != 1 or len(off) < 1 or int(off[-1]) > len(h):
        raise ValueError(f"{name}: rows as CSR (hashes u32[...], row_off u64[n + 1]) expected")
    return h, off


def _pair_slots(ka, kb):
    ka, kb = np.asarray(ka), np.asarray(kb)
    if ka.ndim != 1 or ka.shape != kb.shape:
        raise ValueError("rows intersect: ka and kb are 1-d arrays of one length")
    for k in (ka, kb):
        if len(k) and (k.dtype.kind not in "iu" or int(k.min()) < 0 or int(k.max()) > 0xffffffff):
            raise ValueError("rows intersect: a pair slot is not a row of its set")
    return np.ascontiguousarray(ka, dtype=np.uint32), np.ascontiguousarray(kb, dtype=np.uint32)


def rows_intersect_host(rows_a, rows_b, ka, kb, threads: int = 1) -> np.ndarray:
    """exact row overlaps on the CPU (fdgpu_rows_intersect_host: no context, no device): rows_a / rows_b are CSR pairs (hashes, row_off) as
    FolddiscoIndex.rows, rows_host and RowSet.export return them (rows_b = None: both rows from rows_a) -> inter u32[len(ka)],
    inter[p] = |row ka[p] of rows_a ∩ row kb[p] of rows_b|, in the order of the pairs.  The result does not depend on `threads`.  Raises
    ValueError opening "rows intersect:" for a slot that is not a row of its set or 2^32 pairs"""
    ha, oa = _csr_rows(rows_a, "rows_a")
    hb, ob = (None, None) if rows_b is None else _csr_rows(rows_b, "rows_b")
    ka, kb = _pair_slots(ka, kb)
    L = _lib.load()
    op = u32p()
    rc = L.fdgpu_rows_intersect_host(ha.ctypes.data_as(u32p), oa.ctypes.data_as(u64p), len(oa) - 1, None if hb is None else hb.ctypes.data_as(u32p),
                                     None if ob is None else ob.ctypes.data_as(u64p), 0 if ob is None else len(ob) - 1, ka.ctypes.data_as(u32p),
                                     kb.ctypes.data_as(u32p), len(ka), max(int(threads), 1), C.byref(op))
    if rc != 0:
        raise ValueError(f"rows intersect: fdgpu_rows_intersect_host failed ({rc}): a pair slot at or above its set's row count, offsets that "
                         "descend, or 2^32 or more pairs")
    return _lib.owned_view(L, op, max(len(ka), 1) * 4, np.uint32)[: len(ka)]


def row_overlaps_from_rows(rows_a, rows_b, ka, kb) -> np.ndarray:
    """THE SPECIFICATION of the row overlaps, in plain numpy: np.intersect1d per pair over CSR rows (rows_b = None: both from rows_a) ->
    inter u32[len(ka)].  The device form (Context.rowset_intersect) and the host form (rows_intersect_host) agree with it exactly"""
    ha, oa = _csr_rows(rows_a, "rows_a")
    hb, ob = (ha, oa) if rows_b is None else _csr_rows(rows_b, "rows_b")
    ka, kb = _pair_slots(ka, kb)
    out = np.zeros(len(ka), np.uint32)
    for p, (x, y) in enumerate(zip(ka, kb)):
        out[p] = len(np.intersect1d(ha[int(oa[x]):int(oa[x + 1])], hb[int(ob[y]):int(ob[y + 1])]))
    return out


def jaccard_floor(F: float) -> int:
    """T of a floor F in (0, 1]: round(F * 10^4); ValueError outside (NaN too)"""
    if not 0.0 < float(F) <= 1.0:
        raise ValueError(f"a Jaccard floor of {F} is outside (0, 1]")
    return int(round(float(F) * 10000))


def jaccard_reaches(inter, union, F: float):
    """does a pair reach the floor F?  True if and only if union > 0 and inter * 10^4 >= round(F * 10^4) * union, in 64-bit integers; the one
    expression every form uses.  Scalars give a bool, arrays a bool array"""
    T = np.int64(jaccard_floor(F))
    i, u = np.asarray(inter).astype(np.int64), np.asarray(union).astype(np.int64)
    r = (u > 0) & (i * np.int64(10000) >= T * u)
    return bool(r) if r.ndim == 0 else r


def _overlap_pairs_ids(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 1 or a.shape != b.shape:
        raise ValueError("row overlaps: a and b are 1-d arrays of absolute structure ids, one length")
    for x in (a, b):
        if len(x) and (x.dtype.kind not in "iu" or int(x.min()) < 0 or int(x.max()) > 0xffffffff):
            raise ValueError("row overlaps: an id is not a structure id")
    return a.astype(np.int64), b.astype(np.int64)


def _row_overlap_tiles(take_a, take_b, intersect, a, b, pool_hashes, stats):
    """the tiling both drivers share.  take_x(ids, max_hashes) -> (set, its row lengths, n_taken) extracts a prefix of the ascending ids;
    intersect(A, B, ka, kb) -> inter; sets are released with .close() where they have one"""
    a, b = _overlap_pairs_ids(a, b)
    P = len(a)
    inter, n_a, n_b = np.zeros(P, np.uint32), np.zeros(P, np.uint32), np.zeros(P, np.uint32)
    half = max(int(pool_hashes) // 2, 1)
    ua = np.unique(a)
    st = {"extractions": 0, "distinct": len(ua) + len(np.unique(b)), "tiles": 0}
    pa = 0
    while pa < len(ua):
        A, len_a, ta = take_a(ua[pa:], half)
        st["extractions"] += ta
        ca = ua[pa:pa + ta]
        sel = np.nonzero((a >= ca[0]) & (a <= ca[-1]))[0]         # the pairs of this A chunk
        ub = np.unique(b[sel])
        pb = 0
        while pb < len(ub):
            B, len_b, tb = take_b(ub[pb:], half)
            st["extractions"] += tb
            cb = ub[pb:pb + tb]
            t = sel[(b[sel] >= cb[0]) & (b[sel] <= cb[-1])]       # the pairs of this (A chunk, B chunk) tile
            ka, kb = np.searchsorted(ca, a[t]).astype(np.uint32), np.searchsorted(cb, b[t]).astype(np.uint32)
            inter[t] = intersect(A, B, ka, kb)
            n_a[t], n_b[t] = len_a[ka], len_b[kb]
            st["tiles"] += 1
            if hasattr(B, "close"):
                B.close()
            pb += tb
        if hasattr(A, "close"):
            A.close()
        pa += ta
    if stats is not None:
        stats.update(st)
    return inter, n_a, n_b


def row_overlaps(ix_a, ix_b, a, b, window: int = 16384, pool_hashes: int = OVERLAP_POOL_HASHES, stats=None):
    """exact row overlaps of the pairs (a[p], b[p]) on the device: absolute ids a[p] of the resident index ix_a and b[p] of ix_b (ix_b = None or
    ix_a itself: one index; both on one context) -> (inter, n_a, n_b), u32 arrays in the order of the pairs: the overlap and the two rows'
    sizes (union = n_a + n_b - inter).  At most pool_hashes hashes are resident at a time, half for each side: the distinct ascending a ids
    are taken in chunks (one FolddiscoIndex.rowset call each, advancing by its n_taken), for each A chunk the distinct ascending b ids of
    its pairs in chunks the same way, and the pairs of every (A chunk, B chunk) tile are intersected (Context.rowset_intersect).  The result
    does not depend on pool_hashes or window.  With a small pool a row is extracted more than once — a B row once per A chunk that has a
    pair with it; stats (a dict, if given) receives `extractions`, `distinct` (distinct a ids + distinct b ids) and `tiles`"""
    ix_b = ix_a if ix_b is None else ix_b
    ctx = ix_a.ctx

    def take(ix):
        def f(ids, half):
            rs, t = ix.rowset(ids, window=window, max_hashes=half)
            return rs, rs.lengths(), t
        return f
    return _row_overlap_tiles(take(ix_a), take(ix_b), ctx.rowset_intersect, a, b, pool_hashes, stats)


def _rowset_host(files, ids, window, max_hashes, threads):
    """FolddiscoIndex.rowset over host arrays: files = (value, hashes, offsets, n_structures[, first_id]); the same windows and the same budget
    rule -> ((hashes, row_off), row lengths, n_taken)"""
    value, hashes, offsets, n = files[:4]
    first = int(files[4]) if len(files) > 4 else 0
    window = int(window) or 16384
    pieces, lens, k, total, full = [], [], 0, 0, False
    while k < len(ids) and not full:
        lo = int(ids[k])
        hi = min(lo + window, first + int(n))
        k1 = int(np.searchsorted(ids, hi))
        wh, woff = rows_host(value, hashes, offsets, n, first_id=first, lo=lo, hi=hi, threads=threads)
        t = 0
        for j in range(k, k1):
            s = int(ids[j]) - lo
            r0, r1 = int(woff[s]), int(woff[s + 1])
            if max_hashes and j > 0 and total + (r1 - r0) > max_hashes:
                full = True
                break
            total += r1 - r0
            lens.append(r1 - r0)
            pieces.append(np.array(wh[r0:r1]))
            t += 1
        k += t
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, dtype=np.uint64), dtype=np.uint64)
    return (np.concatenate(pieces).astype(np.uint32, copy=False) if pieces else np.zeros(0, np.uint32), off), np.asarray(lens, dtype=np.uint32), k


def row_overlaps_host(files_a, files_b, a, b, window: int = 16384, pool_hashes: int = OVERLAP_POOL_HASHES, threads: int = 1, stats=None):
    """row_overlaps on the CPU (no context, no device): files_a / files_b = (value, hashes, offsets, n_structures[, first_id]) of the two
    indices (files_b = None: one index).  The same tiles over rows_host windows, so no more than pool_hashes hashes of rows are held at a time;
    the same result, whatever pool_hashes, window and threads are"""
    files_b = files_a if files_b is None else files_b

    def take(files):
        files = (np.ascontiguousarray(files[0], dtype=np.uint8), np.ascontiguousarray(files[1], dtype=np.uint32),
                 np.ascontiguousarray(files[2], dtype=np.uint64)) + tuple(files[3:])
        ids_end = (int(files[4]) if len(files) > 4 else 0) + int(files[3])

        def f(ids, half):
            if len(ids) and (int(ids[0]) < ids_end - int(files[3]) or int(ids[-1]) >= ids_end):
                raise ValueError("row overlaps: an id is outside [first_id, first_id + n_structures)")
            return _rowset_host(files, ids, window, half, threads)
        return f
    return _row_overlap_tiles(take(files_a), take(files_b), lambda A, B, ka, kb: rows_intersect_host(A, B, ka, kb, threads=threads), a, b, pool_hashes, stats)


# ---- exact neighbours (include/fdgpu.h: fd_row_neighbor, fdgpu_rowset_neighbors, fdgpu_rows_neighbors_host) ----------------------------------
# For a query row R_q and structure s of an index D: inter = the number of hashes of R_q whose list in D holds s, union = |R_q| + d_len[s] - inter.
# s is a candidate iff inter > 0, s != exclude[q] and inter * 10^4 >= floor_e4 * union; nearer = the larger inter / union (cross products), then
# the larger inter, then the smaller id.  Integers only.
ROW_NEIGHBOR_DTYPE = np.dtype([("id", "<u4"), ("inter", "<u4"), ("union", "<u4"), ("flags", "<u4")])      # 16 bytes; an empty slot: id = ROW_NO_ID, zeros
ROW_NO_ID = 0xffffffff
ROW_EQUAL = 1                                        # flags bit 0: inter == |R_q| == d_len, the two rows are the same set
ROW_MAX_K = 32
assert ROW_NEIGHBOR_DTYPE.itemsize == 16


def _row_neighbor_args(nQ, S, d_len, k, floor, floor_e4, exclude):
    T = int(floor_e4) if floor is None else jaccard_floor(floor)
    if not (0 <= int(k) <= 0xffffffff and 0 <= T <= 0xffffffff):
        raise ValueError("row neighbors: k must be 1 .. 32 and floor_e4 0 .. 10000")
    d_len = np.ascontiguousarray(d_len, dtype=np.uint32)
    if d_len.shape != (int(S),):
        raise ValueError(f"row neighbors: d_len needs one row length per structure of the index ({S}), got shape {d_len.shape}")
    if exclude is not None:
        exclude = np.ascontiguousarray(exclude, dtype=np.uint32)
        if exclude.shape != (nQ,):
            raise ValueError(f"row neighbors: exclude needs one id per query ({nQ}), got shape {exclude.shape}")
    return d_len, int(k), T, exclude


def row_neighbors_result(L, op, nQ: int, k: int) -> np.ndarray:
    """the library's fd_row_neighbor records as a (nQ, k) array; releases the block"""
    if not nQ:
        if op:
            L.fdgpu_free(op)
        return np.zeros((0, k), ROW_NEIGHBOR_DTYPE)
    return _lib.owned_view(L, op, nQ * k * ROW_NEIGHBOR_DTYPE.itemsize, np.uint8).view(ROW_NEIGHBOR_DTYPE).reshape(nQ, k)


def rows_neighbors_host(q_rows, files_d, d_len, k: int = 8, floor=None, floor_e4: int = 0, exclude=None, threads: int = 1) -> np.ndarray:
    """the exact neighbours on the CPU (fdgpu_rows_neighbors_host: no context, no device): q_rows = the query rows as CSR (hashes, row_off),
    files_d = (value, hashes, offsets, n_structures[, first_id]) of the index D, d_len[s] = the length of the row of D's structure s ->
    (n_queries, k) ROW_NEIGHBOR_DTYPE records, see row_neighbors_from_rows.  The floor is floor_e4 / 10^4, or jaccard_floor(floor) if that is
    given.  The result does not depend on `threads`.  Raises ValueError opening "row neighbors:" for k outside 1 .. 32, floor_e4 above 10000,
    an exclude id outside D, a damaged index, or row lengths that do not belong to the index"""
    qh, qo = _csr_rows(q_rows, "q_rows")
    value, hashes, offsets, S = files_d[:4]
    first = int(files_d[4]) if len(files_d) > 4 else 0
    value, hashes, offsets = np.ascontiguousarray(value, dtype=np.uint8), np.ascontiguousarray(hashes, dtype=np.uint32), np.ascontiguousarray(offsets, dtype=np.uint64)
    nQ = len(qo) - 1
    d_len, k, T, exclude = _row_neighbor_args(nQ, S, d_len, k, floor, floor_e4, exclude)
    L = _lib.load()
    op = C.c_void_p()
    rc = L.fdgpu_rows_neighbors_host(qh.ctypes.data_as(u32p), qo.ctypes.data_as(u64p), nQ, hashes.ctypes.data_as(u32p), offsets.ctypes.data_as(u64p), len(hashes),
                                     value.ctypes.data_as(u8p), len(value), first, int(S), d_len.ctypes.data_as(u32p),
                                     None if exclude is None else exclude.ctypes.data_as(u32p), k, T, max(int(threads), 1), C.byref(op))
    if rc != 0:
        raise ValueError(f"row neighbors: fdgpu_rows_neighbors_host failed ({rc}): k must be 1 .. 32, floor_e4 0 .. 10000, an exclude id is 0xFFFFFFFF or an "
                         "id of the index, the index is sound and d_len holds its rows' lengths")
    return row_neighbors_result(L, op, nQ, k)


def row_neighbors_from_rows(q_rows, d_rows, first_id: int = 0, k: int = 8, floor_e4: int = 0, exclude=None) -> np.ndarray:
    """THE SPECIFICATION of the exact neighbours, in plain Python: sets and a full sort.  q_rows / d_rows: the query rows and ALL rows of D as
    CSR; structure s of D has the id first_id + s -> (n_queries, k) ROW_NEIGHBOR_DTYPE records.  s is a candidate of q iff inter = |R_q ∩ R_s|
    > 0, first_id + s != exclude[q] and inter * 10^4 >= floor_e4 * union (union = |R_q| + |R_s| - inter).  Row q holds q's candidates by
    descending inter / union (as exact fractions), then descending inter, then ascending id, cut at k; the slots behind them are empty
    (id = ROW_NO_ID, zeros).  flags bit 0: inter == |R_q| == |R_s|.  The device form (Context.rowset_neighbors) and the host form
    (rows_neighbors_host) agree with it byte for byte"""
    qh, qo = _csr_rows(q_rows, "q_rows")
    dh, do = _csr_rows(d_rows, "d_rows")
    nQ, S = len(qo) - 1, len(do) - 1
    ds = [frozenset(dh[int(do[s]):int(do[s + 1])].tolist()) for s in range(S)]
    out = np.zeros((nQ, int(k)), ROW_NEIGHBOR_DTYPE)
    out["id"] = ROW_NO_ID
    for q in range(nQ):
        rq = frozenset(qh[int(qo[q]):int(qo[q + 1])].tolist())
        skip = ROW_NO_ID if exclude is None else int(exclude[q])
        cand = []
        for s, rs in enumerate(ds):
            i = len(rq & rs)
            u = len(rq) + len(rs) - i
            if i > 0 and first_id + s != skip and i * 10000 >= int(floor_e4) * u:
                cand.append((-((i << 64) // u), -i, first_id + s, u))      # fractions with denominators below 2^32: distinct -> distinct integers, equal -> equal
        for r, (_, ni, sid, u) in enumerate(sorted(cand)[:int(k)]):
            out[q, r] = (sid, -ni, u, ROW_EQUAL if -ni == len(rq) == len(ds[sid - first_id]) else 0)
    return out


def _row_neighbor_ids(ids):
    ids = np.asarray(ids)
    if ids.ndim != 1 or (len(ids) and (ids.dtype.kind not in "iu" or int(ids.min()) < 0 or int(ids.max()) > 0xffffffff)):
        raise ValueError("row neighbors: ids are absolute structure ids (1-d, below 2^32)")
    ids = ids.astype(np.int64)
    if len(ids) > 1 and not bool((np.diff(ids) > 0).all()):
        raise ValueError("row neighbors: the query ids ascend strictly")
    return ids


def _row_neighbor_chunks(take, neighbors, ids, k, exclude, pool_hashes, stats):
    """the tiling both drivers share: take(ids, max_hashes) -> (query set, n_taken) extracts a prefix of the ascending ids, neighbors(set,
    exclude of the chunk) -> its records; sets are released with .close() where they have one"""
    ids = _row_neighbor_ids(ids)
    if exclude is not None:
        exclude = np.ascontiguousarray(exclude, dtype=np.uint32)
        if exclude.shape != (len(ids),):
            raise ValueError(f"row neighbors: exclude needs one id per query ({len(ids)}), got shape {exclude.shape}")
    out = np.zeros((len(ids), int(k)), ROW_NEIGHBOR_DTYPE)
    at, chunks = 0, 0
    while at < len(ids):
        Q, t = take(ids[at:], max(int(pool_hashes), 1))
        out[at:at + t] = neighbors(Q, None if exclude is None else exclude[at:at + t])
        if hasattr(Q, "close"):
            Q.close()
        at += t
        chunks += 1
    if stats is not None:
        stats.update({"chunks": chunks})
    return out


def row_neighbors(ix_q, ix_d, ids, d_len, k: int = 8, floor_e4: int = 0, exclude=None, window: int = 16384, pool_hashes: int = OVERLAP_POOL_HASHES,
                  counter_bytes: int = 0, stats=None) -> np.ndarray:
    """the exact neighbours of the structures `ids` (absolute, strictly ascending) of the resident index ix_q among the structures of ix_d
    (None or ix_q itself: one index; both on one context), on the device -> (len(ids), k) ROW_NEIGHBOR_DTYPE records.  d_len[s] = the length
    of the row of ix_d's structure s (the n of its signature); exclude[j] (optional) = one id of ix_d that is never a neighbour of ids[j],
    ROW_NO_ID = none.  The query rows are taken in chunks of at most pool_hashes hashes (one FolddiscoIndex.rowset call each, advancing by
    its n_taken) and every chunk is one Context.rowset_neighbors call with a counter table of at most counter_bytes bytes (0: 1 GiB).  The
    result does not depend on pool_hashes, window or counter_bytes"""
    ix_d = ix_q if ix_d is None else ix_d
    ctx = ix_q.ctx
    return _row_neighbor_chunks(lambda rest, pool: ix_q.rowset(rest, window=window, max_hashes=pool),
                                lambda Q, ex: ctx.rowset_neighbors(Q, ix_d, d_len, k=k, floor_e4=floor_e4, exclude=ex, counter_bytes=counter_bytes),
                                ids, k, exclude, pool_hashes, stats)


def row_neighbors_host(files_q, files_d, ids, d_len, k: int = 8, floor_e4: int = 0, exclude=None, window: int = 16384,
                       pool_hashes: int = OVERLAP_POOL_HASHES, threads: int = 1, stats=None) -> np.ndarray:
    """row_neighbors on the CPU (no context, no device): files_q / files_d = (value, hashes, offsets, n_structures[, first_id]) of the two
    indices (files_d = None: one index).  The same chunks over rows_host windows; the same result, whatever pool_hashes, window and threads are"""
    files_d = files_q if files_d is None else files_d
    files_q = (np.ascontiguousarray(files_q[0], dtype=np.uint8), np.ascontiguousarray(files_q[1], dtype=np.uint32),
               np.ascontiguousarray(files_q[2], dtype=np.uint64)) + tuple(files_q[3:])
    first_q = int(files_q[4]) if len(files_q) > 4 else 0

    def take(rest, pool):
        if len(rest) and (int(rest[0]) < first_q or int(rest[-1]) >= first_q + int(files_q[3])):
            raise ValueError("row neighbors: a query id is outside [first_id, first_id + n_structures)")
        rows, _, t = _rowset_host(files_q, rest, window, pool, threads)
        return rows, t
    return _row_neighbor_chunks(take, lambda Q, ex: rows_neighbors_host(Q, files_d, d_len, k=k, floor_e4=floor_e4, exclude=ex, threads=threads),
                                ids, k, exclude, pool_hashes, stats)


# ---- index signatures (include/fdgpu.h: fd_signature, fd_sig_pair) ---------------------------------------------------------------------------
SIGNATURE_DTYPE =np.dtype([("n", "<u4"), ("reserved", "<u4"), ("d0", "<u8"), ("d1", "<u8"), ("sk", "<u4", (64,))])      # 280 bytes
SIGNATURE_PAIR_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("match", "u1"), ("filled", "u1"), ("flags", "<u2")])      # 12 bytes; flags bit 0 = identical
SIGNATURE_PAIRS_DTYPE = np.dtype(SIGNATURE_PAIR_DTYPE.descr + [("estimate", "<f8")])      # what the pair calls return: the record + match / filled
SIG_EMPTY = 0xffffffff
SIG_IDENTICAL = 1
SIG_SEED = 2                                         # flags bit 1 of a cluster record: id is a position in the seed table
assert SIGNATURE_DTYPE.itemsize == 280 and SIGNATURE_PAIR_DTYPE.itemsize == 12


def signature_mix(h) -> np.ndarray:
    """m(h): the splitmix64 finaliser of u32 hashes, as a u64 array"""
    with np.errstate(over="ignore"):
        z = np.asarray(h, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def signatures_from_rows(hashes, row_off) -> np.ndarray:
    """THE SPECIFICATION of the index signatures, in plain numpy: rows as CSR (what FolddiscoIndex.rows / rows_host return) -> one
    SIGNATURE_DTYPE record per row.  With m = signature_mix(h) over the row's distinct hashes: n = their number, d0 = the sum of m mod 2^64,
    d1 = the xor of m, sk[b] = the smallest (m >> 26) & 0xffffffff among the hashes with m >> 58 == b, 0xffffffff for a bucket without one
    (so a value of 0xffffffff in a filled bucket reads as empty, in every form alike).  An empty row: n = d0 = d1 = 0, every sk 0xffffffff.
    The device form (FolddiscoIndex.signatures) and the host form (signatures_host) agree with it bit for bit"""
    hashes = np.asarray(hashes, dtype=np.uint32)
    off = np.asarray(row_off).astype(np.int64)
    out = np.zeros(len(off) - 1, SIGNATURE_DTYPE)
    out["sk"] = SIG_EMPTY
    m = signature_mix(hashes)
    bucket = (m >> np.uint64(58)).astype(np.int64)
    v = ((m >> np.uint64(26)) & np.uint64(0xffffffff)).astype(np.uint32)
    for s in range(len(out)):
        lo, hi = int(off[s]), int(off[s + 1])
        if hi == lo:
            continue
        out["n"][s] = hi - lo
        with np.errstate(over="ignore"):
            out["d0"][s] = np.add.reduce(m[lo:hi], dtype=np.uint64)
        out["d1"][s] = np.bitwise_xor.reduce(m[lo:hi])
        np.minimum.at(out["sk"][s], bucket[lo:hi], v[lo:hi])
    return out


def _sig_table(t, name):
    t = np.ascontiguousarray(t)
    if t.dtype != SIGNATURE_DTYPE or t.ndim != 1:
        raise ValueError(f"{name}: a 1-d array of indexio.SIGNATURE_DTYPE expected")
    return t


def signature_threshold(min_similarity: float) -> int:
    """thr64 of a similarity: ceil(min_similarity * 64), clamped to 1 .. 64"""
    import math
    return max(1, min(64, int(math.ceil(float(min_similarity) * 64))))


def signature_pairs_result(L, pp, n: int) -> np.ndarray:
    """the library's pair records as SIGNATURE_PAIRS_DTYPE (estimate = match / filled, computed here); releases the block"""
    raw = _lib.owned_view(L, pp, n * SIGNATURE_PAIR_DTYPE.itemsize, np.uint8).view(SIGNATURE_PAIR_DTYPE) if n else np.zeros(0, SIGNATURE_PAIR_DTYPE)
    if not n and pp:
        L.fdgpu_free(pp)
    out = np.zeros(n, SIGNATURE_PAIRS_DTYPE)
    for k in SIGNATURE_PAIR_DTYPE.names:
        out[k] = raw[k]
    out["estimate"] = raw["match"].astype(np.float64) / np.maximum(raw["filled"], 1)
    return out


class SignaturePairsOverflow(ValueError):
    """more pairs qualify than max_pairs; .count = how many do"""

    def __init__(self, count: int, max_pairs: int):
        super().__init__(f"signature pairs failed (-4): {count} pairs qualify, more than max_pairs = {max_pairs}; raise the threshold or the cap")
        self.count, self.max_pairs = count, max_pairs


def signatures_host(value, hashes, offsets, n_structures: int, first_id: int = 0, lo=None, hi=None, threads: int = 1) -> np.ndarray:
    """index signatures from host arrays (fdgpu_signatures_host: no context, no device): one SIGNATURE_DTYPE record for each of the structures
    lo .. hi - 1 (absolute ids; default: the whole index), see signatures_from_rows.  The result does not depend on `threads`.  Raises
    ValueError with the library's code in it, as rows_host does"""
    value = np.ascontiguousarray(value, dtype=np.uint8)
    hashes = np.ascontiguousarray(hashes, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offsets) != len(hashes) + 1:
        raise ValueError(f"offsets: {len(hashes) + 1} entries expected, got {len(offsets)}")
    lo = int(first_id) if lo is None else int(lo)
    hi = int(first_id) + int(n_structures) if hi is None else int(hi)
    if lo < 0 or hi < lo:
        raise ValueError("fdgpu_signatures_host failed (-1): lo <= hi, absolute structure ids, expected")
    L = _lib.load()
    op = C.c_void_p()
    rc = L.fdgpu_signatures_host(hashes.ctypes.data_as(u32p), offsets.ctypes.data_as(u64p), len(hashes), value.ctypes.data_as(u8p), len(value), int(first_id),
                                 int(n_structures), lo, hi, max(int(threads), 1), C.byref(op))
    if rc != 0:
        raise ValueError(f"fdgpu_signatures_host failed ({rc}): " + ("a list reaches 4 GiB" if rc == -4 else
                         "the range is not inside the index, or the index is damaged or holds ids outside [first_id, first_id + n_structures)"))
    return _lib.owned_view(L, op, (hi - lo) * SIGNATURE_DTYPE.itemsize, np.uint8).view(SIGNATURE_DTYPE)


def signature_pairs_host(A, B=None, min_similarity: float = 0.9, max_pairs: int = 1 << 24, threads: int = 1, thr64=None) -> np.ndarray:
    """every reported pair of two signature tables on the CPU (fdgpu_signature_pairs_host: no context, no device), sorted by (a, b), as
    SIGNATURE_PAIRS_DTYPE.  B = None: A against itself, a < b only.  A pair is reported iff both rows are non-empty and
    match * 64 >= thr64 * filled with thr64 = signature_threshold(min_similarity) (or the given thr64); estimate = match / filled.  Raises
    SignaturePairsOverflow (with the true count) when more than max_pairs pairs qualify, ValueError for a thr64 outside 1 .. 64"""
    A = _sig_table(A, "A")
    B = None if B is None else _sig_table(B, "B")
    t = signature_threshold(min_similarity) if thr64 is None else int(thr64)
    if not 0 <= t <= 0xffffffff:
        raise ValueError("fdgpu_signature_pairs_host failed (-1): thr64 must be 1 .. 64")
    L = _lib.load()
    pp, n = C.c_void_p(), C.c_uint64()
    rc = L.fdgpu_signature_pairs_host(A.ctypes.data, len(A), None if B is None else B.ctypes.data, 0 if B is None else len(B), t, int(max_pairs),
                                      max(int(threads), 1), C.byref(pp), C.byref(n))
    if rc == -4:
        raise SignaturePairsOverflow(int(n.value), int(max_pairs))
    if rc != 0:
        raise ValueError(f"fdgpu_signature_pairs_host failed ({rc}): thr64 must be 1 .. 64 and a table holds fewer than 2^32 signatures")
    return signature_pairs_result(L, pp, int(n.value))


# ---- signature neighbours (include/fdgpu.h: fd_sig_neighbor)
SIGNATURE_NEIGHBOR_DTYPE = np.dtype([("id", "<u4"), ("match", "u1"), ("filled", "u1"), ("flags", "<u2")])      # 8 bytes; an empty slot: id = SIG_NO_ID, zeros
SIG_NO_ID = 0xffffffff
SIG_MAX_K = 32
assert SIGNATURE_NEIGHBOR_DTYPE.itemsize == 8


def signature_neighbors_from_tables(Q, D=None, k: int = 8, thr64: int = 1, exclude=None) -> np.ndarray:
    """THE SPECIFICATION of the signature neighbours, in plain numpy: -> (len(Q), k) SIGNATURE_NEIGHBOR_DTYPE records.  d of D is a candidate of
    q of Q iff both rows are non-empty, filled > 0 and match * 64 >= thr64 * filled (match = agreeing buckets that are not empty in both,
    filled = 64 - buckets empty in both) and d != exclude[q] (D = None: D is Q and exclude[q] = q).  Row q holds q's candidates by descending
    match / filled, then descending filled, then ascending id, cut at k; the slots behind them are empty (id = SIG_NO_ID, zeros).  flags bit 0:
    n, d0 and d1 agree.  The device form (Context.signature_neighbors) and the host form (signature_neighbors_host) agree with it bit for bit"""
    Q = _sig_table(Q, "Q")
    self_mode = D is None
    D = Q if self_mode else _sig_table(D, "D")
    skip = np.arange(len(Q), dtype=np.int64) if self_mode else np.full(len(Q), SIG_NO_ID, np.int64) if exclude is None else np.asarray(exclude).astype(np.int64)
    out = np.zeros((len(Q), int(k)), SIGNATURE_NEIGHBOR_DTYPE)
    out["id"] = SIG_NO_ID
    d_empty, ids = D["sk"] == SIG_EMPTY, np.arange(len(D), dtype=np.int64)
    for q0 in range(0, len(Q), 128):                 # blocks of queries: 128 x len(D) x 64 booleans at a time
        q = Q[q0:q0 + 128]
        eq = (q["sk"][:, None, :] == D["sk"][None, :, :]).sum(-1)
        E = ((q["sk"] == SIG_EMPTY)[:, None, :] & d_empty[None, :, :]).sum(-1)
        match, filled = eq - E, 64 - E
        ok = (q["n"] > 0)[:, None] & (D["n"] > 0)[None, :] & (filled > 0) & (match * 64 >= int(thr64) * filled) & (ids[None, :] != skip[q0:q0 + 128, None])
        ratio = (match << 20) // np.maximum(filled, 1)      # distinct fractions with denominators <= 64 -> distinct integers, equal -> equal
        for r in range(len(q)):
            c = np.nonzero(ok[r])[0]
            c = c[np.lexsort((c, -filled[r, c], -ratio[r, c]))][:int(k)]
            row = out[q0 + r]
            row["id"][:len(c)], row["match"][:len(c)], row["filled"][:len(c)] = c, match[r, c], filled[r, c]
            row["flags"][:len(c)] = (D["n"][c] == q["n"][r]) & (D["d0"][c] == q["d0"][r]) & (D["d1"][c] == q["d1"][r])
    return out


def _sig_neighbor_args(Q, D, k, min_similarity, thr64, exclude):
    Q = _sig_table(Q, "Q")
    D = None if D is None else _sig_table(D, "D")
    t = int(thr64) if min_similarity is None else signature_threshold(min_similarity)
    if not (0 <= int(k) <= 0xffffffff and 0 <= t <= 0xffffffff):
        raise ValueError("signature neighbors: k must be 1 .. 32 and thr64 1 .. 64")
    if exclude is not None:
        exclude = np.ascontiguousarray(exclude, dtype=np.uint32)
        if exclude.shape != (len(Q),):
            raise ValueError(f"signature neighbors: exclude needs one position per query ({len(Q)}), got shape {exclude.shape}")
    return Q, D, int(k), t, exclude


def signature_neighbors_result(L, op, nQ: int, k: int) -> np.ndarray:
    """the library's neighbour records as a (nQ, k) array; releases the block"""
    if not nQ:
        if op:
            L.fdgpu_free(op)
        return np.zeros((0, k), SIGNATURE_NEIGHBOR_DTYPE)
    return _lib.owned_view(L, op, nQ * k * SIGNATURE_NEIGHBOR_DTYPE.itemsize, np.uint8).view(SIGNATURE_NEIGHBOR_DTYPE).reshape(nQ, k)


def signature_neighbors_host(Q, D=None, k: int = 8, min_similarity=None, thr64: int = 1, exclude=None, threads: int = 1) -> np.ndarray:
    """the k nearest signatures of D for every signature of Q on the CPU (fdgpu_signature_neighbors_host: no context, no device): a (len(Q), k)
    array of SIGNATURE_NEIGHBOR_DTYPE, see signature_neighbors_from_tables.  D = None: inside Q, a signature is never its own neighbour.  The
    floor a neighbour must reach is thr64 / 64, or signature_threshold(min_similarity) if that is given.  The result does not depend on
    `threads`.  Raises ValueError for k outside 1 .. 32, thr64 outside 1 .. 64 and exclude together with D = None"""
    Q, D, k, t, exclude = _sig_neighbor_args(Q, D, k, min_similarity, thr64, exclude)
    L = _lib.load()
    op = C.c_void_p()
    rc = L.fdgpu_signature_neighbors_host(Q.ctypes.data, len(Q), None if D is None else D.ctypes.data, 0 if D is None else len(D),
                                          None if exclude is None else exclude.ctypes.data, k, t, max(int(threads), 1), C.byref(op))
    if rc != 0:
        raise ValueError(f"signature neighbors: fdgpu_signature_neighbors_host failed ({rc}): k must be 1 .. 32, thr64 1 .. 64, a table holds fewer "
                         "than 2^32 signatures and exclude is not given in self mode")
    return signature_neighbors_result(L, op, len(Q), k)


# ---- signature clusters (include/fdgpu.h: fdgpu_signature_clusters); the records are SIGNATURE_NEIGHBOR_DTYPE, one per position
CLUSTER_ORDER_KEYS = ("hashes", "nres", "plddt", "id")


def _sig_cluster_args(S, order, min_similarity, thr64):
    S = _sig_table(S, "S")
    t = signature_threshold(min_similarity) if thr64 is None else int(thr64)
    if not 0 <= t <= 0xffffffff:
        raise ValueError("signature clusters: thr64 must be 1 .. 64")
    if order is not None:
        o = np.asarray(order)
        if o.shape != (len(S),) or o.dtype.kind not in "iu" or (len(o) and (int(o.min()) < 0 or int(o.max()) > 0xffffffff)):
            raise ValueError(f"signature clusters: order needs one position per signature ({len(S)}), each of them 0 .. n - 1")
        order = np.ascontiguousarray(o, dtype=np.uint32)
    return S, order, t


def signature_clusters_from_tables(S, order=None, thr64: int = 58, seeds=None) -> np.ndarray:
    """THE SPECIFICATION of the signature clusters, in plain numpy: -> len(S) SIGNATURE_NEIGHBOR_DTYPE records.  The positions are visited in
    `order` (a permutation of them; None: position order).  A position with an empty row (n = 0) is unclustered: id = SIG_NO_ID and zeros.
    Any other position p looks at the representatives chosen so far that it would be reported with at thr64 (both rows non-empty, filled > 0,
    match * 64 >= thr64 * filled).  None: p becomes a representative, its record is (p, its non-empty buckets twice, SIG_IDENTICAL).  Otherwise p
    joins the nearest of them (descending match / filled, then descending filled, then ascending position in the table): (r, match, filled,
    n, d0 and d1 agree).  seeds: a second table T whose records with n > 0 are representatives before the walk starts, all of them, whether
    or not two of them would be reported together.  The order then runs over combined ids, seed j as j and position p of S as len(T) + p, so
    a seed wins a full tie against a representative of S; a record whose nearest is a seed holds the seed's position in T and SIG_SEED in its
    flags.  Without non-empty seeds the records are those of the unseeded walk.  The device form (Context.signature_clusters) and the host
    form (signature_clusters_host) agree with it byte for byte"""
    S = _sig_table(S, "S")
    n = len(S)
    order = np.arange(n, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)
    if order.shape != (n,) or not np.array_equal(np.sort(order), np.arange(n)):
        raise ValueError(f"signature clusters: order is not a permutation of 0 .. {n - 1}")
    if not 1 <= int(thr64) <= 64:
        raise ValueError("signature clusters: thr64 must be 1 .. 64")
    T = S[:0] if seeds is None else _sig_table(seeds, "seeds")
    nT = len(T)
    if nT + n > 0xffffffff:
        raise ValueError("signature clusters: the seeds and the table together hold more than 2^32 - 1 signatures")
    X = np.concatenate([T, S]) if nT else S          # the combined id space: the seeds, then S
    out = np.zeros(n, SIGNATURE_NEIGHBOR_DTYPE)
    out["id"] = SIG_NO_ID
    empty = X["sk"] == SIG_EMPTY
    reps = np.zeros(nT + n, np.int64)
    n_reps = int((T["n"] > 0).sum())
    reps[:n_reps] = np.nonzero(T["n"] > 0)[0]
    for p in order.tolist():
        if S["n"][p] == 0:
            continue
        x = nT + p
        r = reps[:n_reps]
        eq = (X["sk"][r] == X["sk"][x]).sum(-1)
        E = (empty[r] & empty[x]).sum(-1)
        match, filled = eq - E, 64 - E
        c = np.nonzero((filled > 0) & (match * 64 >= int(thr64) * filled))[0]
        if not len(c):
            k = 64 - int(empty[x].sum())
            out[p] = (p, k, k, SIG_IDENTICAL)
            reps[n_reps] = x
            n_reps += 1
            continue
        ratio = (match[c] << 20) // np.maximum(filled[c], 1)      # as in signature_neighbors_from_tables
        b = c[np.lexsort((r[c], -filled[c], -ratio))[0]]
        q = int(r[b])
        same = int(X["n"][q] == X["n"][x] and X["d0"][q] == X["d0"][x] and X["d1"][q] == X["d1"][x])
        out[p] = (q, match[b], filled[b], same | SIG_SEED) if q < nT else (q - nT, match[b], filled[b], same)
    return out


def signature_clusters_result(L, op, n: int) -> np.ndarray:
    """the library's cluster records as an array of n; releases the block"""
    if not n:
        if op:
            L.fdgpu_free(op)
        return np.zeros(0, SIGNATURE_NEIGHBOR_DTYPE)
    return _lib.owned_view(L, op, n * SIGNATURE_NEIGHBOR_DTYPE.itemsize, np.uint8).view(SIGNATURE_NEIGHBOR_DTYPE)


def signature_clusters_host(S, order=None, min_similarity: float = 0.9, thr64=None, threads: int = 1, seeds=None) -> np.ndarray:
    """the greedy clusters of a signature table on the CPU (fdgpu_signature_clusters_host: no context, no device): one
    SIGNATURE_NEIGHBOR_DTYPE record per position, see signature_clusters_from_tables.  The threshold is thr64 / 64 if thr64 is given, else
    signature_threshold(min_similarity).  seeds: a signature table whose non-empty records are representatives from the start
    (fdgpu_signature_clusters_seeded_host).  The result does not depend on `threads`.  Raises ValueError for a thr64 outside 1 .. 64 and an
    order that is not a permutation of the positions"""
    S, order, t = _sig_cluster_args(S, order, min_similarity, thr64)
    L = _lib.load()
    op = C.c_void_p()
    if seeds is not None:
        T = _sig_table(seeds, "seeds")
        rc = L.fdgpu_signature_clusters_seeded_host(S.ctypes.data, len(S), None if order is None else order.ctypes.data, T.ctypes.data if len(T) else None,
                                                    len(T), t, max(int(threads), 1), C.byref(op))
        if rc != 0:
            raise ValueError(f"signature clusters: fdgpu_signature_clusters_seeded_host failed ({rc}): thr64 must be 1 .. 64, the seeds and the table "
                             "together hold fewer than 2^32 - 1 signatures and order is a permutation of 0 .. n - 1")
        return signature_clusters_result(L, op, len(S))
    rc = L.fdgpu_signature_clusters_host(S.ctypes.data, len(S), None if order is None else order.ctypes.data, t, max(int(threads), 1), C.byref(op))
    if rc != 0:
        raise ValueError(f"signature clusters: fdgpu_signature_clusters_host failed ({rc}): thr64 must be 1 .. 64, the table holds fewer than 2^32 "
                         "signatures and order is a permutation of 0 .. n - 1")
    return signature_clusters_result(L, op, len(S))


def cluster_order(S, lookup_rows, by: str = "hashes") -> np.ndarray:
    """the walk orders of `cluster` -> the positions in the order they are visited (u32).  by = "hashes": the signature's n, descending (the
    most complete structure represents); "nres" / "plddt": that column of PREFIX.lookup, descending; "id": ascending.  Ties go by ascending
    id.  ValueError for another key, a row count that is not len(S), or a row with fewer than four columns"""
    if by not in CLUSTER_ORDER_KEYS:
        raise ValueError(f"unknown representative key '{by}' (one of {', '.join(CLUSTER_ORDER_KEYS)})")
    n = len(S)
    if by == "id":
        return np.arange(n, dtype=np.uint32)
    if by == "hashes":
        key = np.asarray(S["n"]).astype(np.float64)
    else:
        if len(lookup_rows) != n:
            raise ValueError(f".lookup holds {len(lookup_rows)} rows, the table {n} signatures")
        cols = [r.rstrip("\n").split("\t") for r in lookup_rows]
        if any(len(c) < 4 for c in cols):
            raise ValueError("a .lookup row has fewer than four columns")
        key = np.array([float(int(c[2])) if by == "nres" else float(c[3]) for c in cols], np.float64).reshape(n)
    return np.lexsort((np.arange(n), -key)).astype(np.uint32)


def permute_lookup_rows(rows, new_id, keep_db_keys: bool):
    """the rows of PREFIX.lookup after a reorder: row k moves to position new_id[k], tid, nres and plddt verbatim, the id renumbered 0 .. n - 1; the
    db_key column renumbered with it for a file-built index (there it equals the id) and kept for a Foldcomp-built one (its database key) -- the
    convention of update_lookup_rows"""
    p = np.asarray(new_id, dtype=np.int64)
    n = len(rows)
    if p.ndim != 1 or len(p) != n or (n and not np.array_equal(np.sort(p), np.arange(n))):
        raise ValueError(f"new_id: a permutation of 0 .. {n - 1} expected")
    out = [None] * n
    for row, i in zip(rows, p.tolist()):
        c = row.rstrip("\n").split("\t")
        c[0] = str(i)
        if len(c) > 4 and not keep_db_keys:
            c[4] = str(i)
        out[i] = "\t".join(c) + "\n"
    return out


ORDER_KEYS = ("tid", "nres", "plddt")


def order_from_lookup(rows, by=None, descending: bool = False, order_tids=None) -> np.ndarray:
    """the ordering rules of `reorder` -> new_id (new_id[k] = new position of row k).  by: rows sorted by one column of PREFIX.lookup, tid as a byte
    string, nres and plddt numerically; the sort is stable (ties keep their old order) and descending reverses the key, not the tie order.
    order_tids: the tids in their new order; ValueError unless it names every tid of the rows exactly once and the rows hold no tid twice.
    Exactly one of by / order_tids must be given."""
    if (by is None) == (order_tids is None):
        raise ValueError("give exactly one of a sort key (--by) and a list of tids (--order)")
    n = len(rows)
    cols = [r.rstrip("\n").split("\t") for r in rows]
    if any(len(c) < 4 for c in cols):
        raise ValueError("a .lookup row has fewer than four columns")
    if by is not None:
        if by not in ORDER_KEYS:
            raise ValueError(f"unknown sort key '{by}' (one of {', '.join(ORDER_KEYS)})")
        if by == "tid":
            keys = [c[1].encode("utf-8", "surrogateescape") for c in cols]
        elif by == "nres":
            keys = [int(c[2]) for c in cols]
        else:
            keys = [float(c[3]) for c in cols]
        ranked = sorted(range(n), key=lambda k: keys[k], reverse=descending)      # stable; reverse=True keeps ties in their old order too
        new_id = np.empty(n, np.uint32)
        new_id[np.asarray(ranked, dtype=np.int64)] = np.arange(n, dtype=np.uint32)
        return new_id
    where = {}
    for k, c in enumerate(cols):
        if c[1] in where:
            raise ValueError(f"tid '{c[1]}' appears twice in .lookup (rows {where[c[1]] + 1} and {k + 1}): an order by tid would be ambiguous")
        where[c[1]] = k
    new_id = np.full(n, n, np.int64)
    for pos, t in enumerate(order_tids):
        k = where.get(t)
        if k is None:
            raise ValueError(f"the order names tid '{t}' (line {pos + 1}), which .lookup does not hold")
        if new_id[k] != n:
            raise ValueError(f"the order names tid '{t}' twice (lines {int(new_id[k]) + 1} and {pos + 1})")
        new_id[k] = pos
    if len(order_tids) != n:
        missing = next(cols[k][1] for k in range(n) if new_id[k] == n)
        raise ValueError(f"the order names {len(order_tids)} of {n} tids; '{missing}' is missing")
    return new_id.astype(np.uint32)


def join_lookup_rows(list_of_rows, keep_db_keys: bool):
    """the rows of PREFIX.lookup after a join of indices (`merge`): the inputs' rows in the order given, tid, nres and plddt verbatim, the id
    renumbered densely across the inputs; the db_key column renumbered with it for file-built indices (there it equals the id) and kept for
    Foldcomp-built ones (its database key) -- the convention of update_lookup_rows"""
    out, i = [], 0
    for rows in list_of_rows:
        for row in rows:
            p = row.rstrip("\n").split("\t")
            p[0] = str(i)
            if len(p) > 4 and not keep_db_keys:
                p[4] = str(i)
            out.append("\t".join(p) + "\n")
            i += 1
    return out


def _type_lines(text: str) -> dict:
    """key -> the whole line of a PREFIX.type text (lines without '=' are ignored, like load_type)"""
    return {line.split("=", 1)[0].strip(): line.rstrip("\n") for line in text.splitlines() if "=" in line}


def check_joinable(type_texts):
    """can the indices with these PREFIX.type texts be joined?  Every line but chunk_size must be the same text in all of them (hash type, bins,
    grid width, input format, foldcomp_db, ...): -> the key of the first line that disagrees with the first text (in the first text's order, then
    keys only a later text has), or None"""
    first, others = _type_lines(type_texts[0]), [_type_lines(t) for t in type_texts[1:]]
    keys = list(first) + list(dict.fromkeys(k for o in others for k in o if k not in first))
    for k in keys:
        if k != "chunk_size" and any(first.get(k) != o.get(k) for o in others):
            return k
    return None


# ---- PREFIX.coords: the database's coordinates beside its index (this project's own file) ----------------------------------
# 64-byte header: magic FDCOORD1 | u32 version = 1 | u32 flags (bit 0: cb_valid present) | u64 n_struct | u64 n_res | stamp u64[3] (rows of
# PREFIX.lookup, bytes of PREFIX, bytes of PREFIX.offset when the store was written) | zero padding.  Then, each on a 64-byte boundary:
# res_off u64[S + 1] | n_xyz, ca_xyz, cb_xyz f32[3R] each | aa u8[R] | cb_valid u8[R] (flag bit 0) | resname_std u8[R] | chain u8[R] | serial u64[R].
# Little-endian, section-major (an id range or one structure is one read per section), bytes verbatim from the ingest (fd_parsed).
COORDS_MAGIC = b"FDCOORD1"
COORDS_VERSION = 1
COORDS_HEADER = 64
COORDS_SECTIONS = (("res_off", np.uint64, None), ("n_xyz", np.float32, 3), ("ca_xyz", np.float32, 3), ("cb_xyz", np.float32, 3), ("aa", np.uint8, 1),
                   ("cb_valid", np.uint8, 1), ("resname_std", np.uint8, 1), ("chain", np.uint8, 1), ("serial", np.uint64, 1))
STAMP_FIELDS = ("lookup rows", "value file bytes", "offset file bytes")      # PREFIX.lookup, PREFIX, PREFIX.offset


class CoordStoreError(ValueError):
    """a PREFIX.coords file a reader refuses: inconsistent in itself, or written for other index files than the ones beside it"""


def _pad64(n: int) -> int:
    return (n + 63) & ~63


def _coords_layout(S: int, R: int, with_cbv: bool):
    """-> ({section: (byte offset, elements)}, file size)"""
    pos, lay = COORDS_HEADER, {}
    for name, dt, per in COORDS_SECTIONS:
        if name == "cb_valid" and not with_cbv:
            continue
        n = S + 1 if per is None else per * R
        lay[name] = (pos, n)
        pos = _pad64(pos + n * np.dtype(dt).itemsize)
    last = COORDS_SECTIONS[-1]
    return lay, lay[last[0]][0] + lay[last[0]][1] * np.dtype(last[1]).itemsize      # no padding behind the last section


def index_stamp(prefix: str):
    """what a store remembers of the index files beside it: (rows of PREFIX.lookup, bytes of PREFIX, bytes of PREFIX.offset)"""
    with open(prefix + ".lookup", "rb") as f:
        rows = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 20), b""))
    vp = prefix + ".value" if os.path.exists(prefix + ".value") else prefix
    return rows, os.path.getsize(vp), os.path.getsize(prefix + ".offset")


@dataclass
class CoordArrays:
    """a run of structures as flat arrays: the batch (PackedStructures) and the per-residue labels the result printer needs"""
    ps: object              # api.PackedStructures
    chain: np.ndarray       # u8 [R]
    resname_std: np.ndarray  # u8 [R]
    serial: np.ndarray      # u64 [R]


class _StructView:
    """one structure of a CoordStore as query.query_pdb reads it: views, nothing copied"""
    __slots__ = ("ca_xyz", "chain", "serial")

    def __init__(self, ca_xyz, chain, serial):
        self.ca_xyz, self.chain, self.serial = ca_xyz, chain, serial

    @property
    def n(self) -> int:
        return len(self.chain)


class _LazyStructs:
    """the structures [lo, hi) of a CoordStore as a sequence: len, truthiness, [k]; no per-structure or per-residue object exists before [k] asks"""

    def __init__(self, store, lo, hi):
        self.store, self.lo, self.hi = store, lo, hi

    def __len__(self):
        return self.hi - self.lo

    def __bool__(self):
        return self.hi > self.lo

    def __getitem__(self, k):
        k = int(k)
        if k < 0:
            k += len(self)
        if not 0 <= k < len(self):
            raise IndexError(k)
        st = self.store
        a, b = int(st.res_off[self.lo + k]), int(st.res_off[self.lo + k + 1])
        return _StructView(st.ca_xyz[a:b], st.chain[a:b], st.serial[a:b])

    def __iter__(self):
        return (self[k] for k in range(len(self)))

    def resname_std_all(self) -> np.ndarray:
        st = self.store
        return st.resname_std[int(st.res_off[self.lo]):int(st.res_off[self.hi])]


class CoordStore:
    """PREFIX.coords, memory-mapped read-only.  Arrays: res_off u64[S + 1]; n_xyz, ca_xyz, cb_xyz f32[R, 3]; aa, resname_std, chain u8[R];
    cb_valid u8[R] or None; serial u64[R]; stamp = the three numbers of index_stamp at the time of writing."""

    @staticmethod
    def open(path: str, check_prefix: str | None = None) -> "CoordStore":
        """refuses (CoordStoreError) a store whose header, section sizes or res_off are inconsistent, and — with check_prefix — one whose stamp
        disagrees with the index files at that prefix; OSError for a file that cannot be read"""
        self = CoordStore()
        self.path = path
        size = os.path.getsize(path)
        if size < COORDS_HEADER:
            raise CoordStoreError(f"{path}: {size} bytes, shorter than the {COORDS_HEADER}-byte header")
        mm = np.memmap(path, dtype=np.uint8, mode="r")
        if bytes(mm[:8]) != COORDS_MAGIC:
            raise CoordStoreError(f"{path}: not a coordinate store (magic {bytes(mm[:8])!r})")
        ver, flags = (int(x) for x in mm[8:16].view("<u4"))
        if ver != COORDS_VERSION:
            raise CoordStoreError(f"{path}: version {ver}, this reader knows version {COORDS_VERSION}")
        if flags & ~1:
            raise CoordStoreError(f"{path}: unknown flag bits {flags:#x}")
        S, R, *stamp = (int(x) for x in mm[16:56].view("<u8"))
        if S >= 0xffffffff or R >= 1 << 48:
            raise CoordStoreError(f"{path}: header claims {S} structures and {R} residues")
        lay, want = _coords_layout(S, R, bool(flags & 1))
        if size != want:
            raise CoordStoreError(f"{path}: {size} bytes, its header ({S} structures, {R} residues) asks for exactly {want}"
                                  + (" (truncated)" if size < want else " (trailing bytes)"))
        self.n_struct, self.n_res, self.stamp, self.flags = S, R, tuple(stamp), flags
        for name, dt, per in COORDS_SECTIONS:
            if name not in lay:
                setattr(self, name, None)
                continue
            pos, n = lay[name]
            arr = mm[pos:pos + n * np.dtype(dt).itemsize].view(np.dtype(dt).newbyteorder("<"))
            setattr(self, name, arr.reshape(-1, 3) if per == 3 else arr)
        off = self.res_off
        if int(off[0]) != 0:
            raise CoordStoreError(f"{path}: res_off[0] is {int(off[0])}, not 0")
        if S and not bool(np.all(off[1:] >= off[:-1])):
            k = int(np.nonzero(off[1:] < off[:-1])[0][0])
            raise CoordStoreError(f"{path}: res_off does not ascend (structure {k}: {int(off[k])} -> {int(off[k + 1])})")
        if int(off[S]) != R:
            raise CoordStoreError(f"{path}: res_off[{S}] is {int(off[S])}, the header says {R} residues")
        if check_prefix is not None:
            self.check_stamp(check_prefix)
        return self

    def check_stamp(self, prefix: str):
        now = index_stamp(prefix)
        for name, was, isnow in zip(STAMP_FIELDS, self.stamp, now):
            if was != isnow:
                raise CoordStoreError(f"{self.path} was written for other index files than those at {prefix}: {name} = {was} in its stamp, {isnow} now "
                                      f"(rebuild it with `coords -i {prefix}`)")

    def _arrays(self, sl, off) -> CoordArrays:
        from .api import PackedStructures
        take = lambda a: None if a is None else a[sl]
        return CoordArrays(PackedStructures(off, take(self.n_xyz), take(self.ca_xyz), take(self.cb_xyz), take(self.aa), take(self.cb_valid)),
                           take(self.chain), take(self.resname_std), take(self.serial))

    def slice(self, lo: int, hi: int) -> CoordArrays:
        """structures [lo, hi): views of the mapping (res_off rebased to 0 is the one copy)"""
        if not 0 <= lo <= hi <= self.n_struct:
            raise IndexError(f"slice [{lo}, {hi}) of {self.n_struct} structures")
        a, b = int(self.res_off[lo]), int(self.res_off[hi])
        return self._arrays(slice(a, b), np.asarray(self.res_off[lo:hi + 1]) - np.uint64(a))

    def select(self, ids) -> CoordArrays:
        """structure k of the result = structure ids[k] of the store (a gather: any order, repeats allowed); copies"""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if len(ids) and (ids.min() < 0 or ids.max() >= self.n_struct):
            raise IndexError(f"select: ids outside 0 .. {self.n_struct - 1}")
        start = np.asarray(self.res_off)[ids].astype(np.int64)
        lens = np.asarray(self.res_off)[ids + 1].astype(np.int64) - start
        off = np.zeros(len(ids) + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        idx = np.repeat(start - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]), dtype=np.int64)
        return self._arrays(idx, off)

    def structs(self, lo: int = 0, hi: int | None = None) -> _LazyStructs:
        hi = self.n_struct if hi is None else hi
        if not 0 <= lo <= hi <= self.n_struct:
            raise IndexError(f"structs [{lo}, {hi}) of {self.n_struct} structures")
        return _LazyStructs(self, lo, hi)


class CoordWriter:
    """streams a store: add() appends runs of structures to one temporary file per section, close(stamp) assembles header and sections under a
    temporary name and renames it to `path`; abort() (or a failed close) leaves nothing behind.  write_coords is the whole of it in one call."""
    BLOCK = 1 << 16      # structures per gathered block of a (store, ids) piece

    def __init__(self, path: str):
        self.path, self.tmp = path, f"{path}.tmp{os.getpid()}"
        self.S = self.R = 0
        self.cbv_seen = self.cbv_missing = False
        self.files = {name: open(f"{self.tmp}.{name}", "wb") for name, _, _ in COORDS_SECTIONS}
        self.files["res_off"].write(np.zeros(1, "<u8").tobytes())

    def _add_arrays(self, a: CoordArrays):
        ps = a.ps
        n = int(ps.res_off[-1])
        if not (len(a.chain) == len(a.resname_std) == len(a.serial) == n):
            raise ValueError("write_coords: label arrays do not match res_off[-1]")
        put = lambda name, arr, dt: self.files[name].write(np.ascontiguousarray(arr, dtype=np.dtype(dt).newbyteorder("<")).tobytes())
        put("res_off", np.asarray(ps.res_off[1:], np.uint64) + np.uint64(self.R), np.uint64)
        for name in ("n_xyz", "ca_xyz", "cb_xyz"):
            put(name, getattr(ps, name), np.float32)
        put("aa", ps.aa, np.uint8)
        if ps.cb_valid is None:
            self.cbv_missing = self.cbv_missing or n > 0
            put("cb_valid", np.ones(n, np.uint8), np.uint8)      # a piece without cb_valid contributes ones when another piece has it
        else:
            self.cbv_seen = True
            put("cb_valid", ps.cb_valid, np.uint8)
        put("resname_std", a.resname_std, np.uint8)
        put("chain", a.chain, np.uint8)
        put("serial", a.serial, np.uint64)
        self.S += ps.n_struct
        self.R += n

    def add(self, piece):
        """piece: CoordArrays (raw arrays), or (CoordStore, ids or None) — the structures ids[k] of the store in that order, None = all of it"""
        if isinstance(piece, CoordArrays):
            return self._add_arrays(piece)
        store, ids = piece
        if ids is None:
            for lo in range(0, store.n_struct, self.BLOCK):
                self._add_arrays(store.slice(lo, min(lo + self.BLOCK, store.n_struct)))
        else:
            ids = np.asarray(ids, dtype=np.int64).reshape(-1)
            for lo in range(0, len(ids), self.BLOCK):
                self._add_arrays(store.select(ids[lo:lo + self.BLOCK]))

    def abort(self):
        for f in self.files.values():
            f.close()
        for p in [f"{self.tmp}.{name}" for name, _, _ in COORDS_SECTIONS] + [self.tmp]:
            if os.path.exists(p):
                os.remove(p)

    def close(self, stamp):
        import shutil
        try:
            for f in self.files.values():
                f.close()
            with_cbv = self.cbv_seen or not self.cbv_missing      # absent only when no piece that has residues carried it
            lay, size = _coords_layout(self.S, self.R, with_cbv)
            head = COORDS_MAGIC + np.array([COORDS_VERSION, 1 if with_cbv else 0], "<u4").tobytes() + \
                np.array([self.S, self.R] + [int(x) for x in stamp], "<u8").tobytes()
            with open(self.tmp, "wb") as out:
                out.write(head.ljust(COORDS_HEADER, b"\0"))
                for name, dt, _ in COORDS_SECTIONS:
                    if name not in lay:
                        continue
                    out.write(b"\0" * (lay[name][0] - out.tell()))
                    with open(f"{self.tmp}.{name}", "rb") as src:
                        shutil.copyfileobj(src, out, 1 << 22)
                    if out.tell() != lay[name][0] + lay[name][1] * np.dtype(dt).itemsize:
                        raise IOError(f"write_coords: section {name} has {out.tell() - lay[name][0]} bytes")
                if out.tell() != size:
                    raise IOError("write_coords: size mismatch")
            os.replace(self.tmp, self.path)
        finally:
            self.abort()


def write_coords(path: str, pieces, stamp):
    """the one writer of PREFIX.coords (`index --coords`, `coords`, `update`, `merge`, `reorder`): the pieces one after the other — each
    (CoordStore, ids or None) or CoordArrays, see CoordWriter.add; pieces may be a generator — streamed to a temporary name and renamed at the
    end.  stamp: the three numbers of index_stamp, or a callable that gives them once the pieces are consumed."""
    w = CoordWriter(path)
    try:
        for p in pieces:
            w.add(p)
    except BaseException:
        w.abort()
        raise
    w.close(stamp() if callable(stamp) else stamp)
