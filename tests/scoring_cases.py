"""Hand-made posting lists for the ranked scoring (count_query_batch / count_query_maps) at the places where its forms can disagree, with a plain
integer model of the scoring that is exact to the bit.  No GPU, nothing committed as data: every index is generated (deterministic seeds) and encoded
with the pure-Python LEB128 codec of rebase_cases.py.

The index shape: S = 5 * 16384 + 3 * 2048 + 37 = 88,101 structures = six tiles of 2^14, 44 checkpoint cells of 2^11 (the last tile: three cells and
a partial one), S no multiple of 32; the ids start at each of FIRST_IDS (0; 3000; 2^28 - 40,000: list heads of four and five bytes in one index;
2^32 - 1 - S: the largest value fdgpu_index_set_first_id accepts).  Lists are written with ids RELATIVE to first_id (negative and >= S: outside the
index's range, kept only where the absolute id fits 32 bits).

The model (model_full / model_count): units of 2^-22, fix = (uint64)(idf * 4194304.0 + 0.5) for 0 < idf < 1e6 else 0 with idf = log2f(f32(total) /
f32(len)) through libm, len = ALL postings of the row's list; per structure in range: hit rows, distinct nodes, distinct (node, edge) pairs, the
integer sum of fix, idf = f32(sum / 2^22) * f32(penalty); ranked = idf descending (-0 as +0), ties by ascending id (np.lexsort), cut to top_n.

Case classes (CLASSES; every case names its class and carries the property it claims as data in `claims`, which test_scoring_cases_host.py checks):
  stride  byte lengths one below and at every threshold 48 * ceil(44 / 2^j) of the checkpoint stride (96, 144, 288, 528, 1056, 2112), each list with
          ids in all six tiles; the dense list of every id; lists that leave whole tiles empty, the last ones included (boundaries behind the last
          posting); one-posting lists at 0, 2047, 2048, 16383, 16384 and S - 1.
  carry   lists (>= 2112 bytes: an entry per cell) in which a 2-, 3- or 5-byte varint straddles byte 64 k of the LIST (the checkpoint fill walks a
          list in 64-byte blocks from its first byte, so the list's head itself never straddles one) and is the first posting at or behind a cell
          boundary.  Five-byte varints inside a list need a step of >= 2^28: from an id below first_id into the range (first_id >= 2^28 - 40,000),
          or from the range to an id beyond it (first_id + S + 2^28 < 2^32).
  slots   cells of 1023, 1024, 1025 and 2048 one-byte postings (pieces of 64, 65 and 128 slots of 16 bytes); single-piece lists whose last varint
          ends on byte 15 / 16 / 17 of a slot, as a 1-, 2- and 3-byte varint; varints of 2, 3 and 5 bytes that straddle a slot boundary with 1 to 4
          bytes in the slot before (the decoder's look-back); queries whose pieces in every tile sum to 63, 64 and 65 slots before a piece of 2 slots
          arrives (next-fit opens a window or not).
  ties    penalty 1.0; structures 16380 .. 16390 and 32760 .. 32775 hit by exactly the same rows, top_n cuts inside the runs; runs placed so that one
          tile holds exactly top_n equal keys and its neighbour top_n + 1.
  crowd   top_n = 50 (the selection holds cap = 1074): 1073, 1074 and 1075 structures with one identical key at the cut plus one lower key in the same
          first-level bin (direct threshold, second level, overflow to the compacting path); the same with keys one or two f32 ulps apart inside one
          64-key sub-bin; the cut in bin 0 (penalty 0.0 for 3,000 hit structures, -0.0 and negative ones for some); the cut in bin 2047 (idf > 2^16).
  width   idf units next to the 32-bit accumulator's end: total_structures = 2^31, 32 rows of one posting, one of 32768 and one of 32769, one structure in
          all 34 lists (sum 2^32 - 184); with a second list of 32768 instead: exactly 2^32; a row whose idf is 0 units (a list of all S ids, total = S) with
          structures hit by that row only; total_structures = 2^33 with a one-posting list (fix >= 2^27: no packed accumulators).
  rows    kept rows per query of 128 / 129 (query maps: which of the map's hashes the index holds) and a batch that mixes a 129-row query with 5-row
          ones; 1024 / 1025 rows and, as a single query, 4095 / 4096 rows over a 4,200-list index.
  groups  free (node, edge) rows: 1,000 rows whose edge groups end at positions 31, 32 and 33 of a 32-row word, a group over three words, single-row
          groups, all rows on one node; structures hit only by non-end rows of a group, only by its end row, and by a row of every group; rows given
          out of (node, edge) order.
  shard   lists with ids below first_id and at or above first_id + S on both ends, and a list wholly outside the range.

Cases run as free rows (`via == "batch"`: count_query_batch, hash 3 k + 1 for list k) or through query maps (`via == "maps"`: list k sits on the k-th
distinct hash of a real motif's map, the rows are the map's (hash, qi, qj)); map_variants() restates every small batch case as map cases, since the
32-bit form and its slot windows are reached through maps only."""
import ctypes as C

import numpy as np

from tests.rebase_cases import decode, encode, varint  # noqa: F401  (the codec of the hand-made indices)

S = 5 * 16384 + 3 * 2048 + 37
CELL_LOG2, TILE_LOG2 = 11, 14
NC, NT = (S + 2047) >> 11, (S + 16383) >> 14
FIRST_IDS = (0, 3000, (1 << 28) - 40000, 0xffffffff - S)
STRIDE_THRESHOLDS = (96, 144, 288, 528, 1056, 2112)
CLASSES = ("stride", "carry", "slots", "ties", "crowd", "width", "rows", "groups", "shard")
REC = np.dtype([("nid", np.uint32), ("total_match_count", np.uint32), ("node_count", np.uint32), ("edge_count", np.uint32), ("idf", np.float32)])
SEED = 20261018
# the motif the map cases sit on: residues B18 .. B24 of tests/golden/query/4CHA.pdb, the first of the shortest contiguous runs of residues (seven) whose
# query map has at least 160 entries — it has exactly 160, all with distinct hashes; the small map of the mixed batches: its first two residues (8 entries)
MOTIF, MOTIF_SMALL = "B18-24", "B18-19"
MAX_MAP_ROWS = 160

_libm = C.CDLL("libm.so.6")
_libm.log2f.restype = C.c_float
_libm.log2f.argtypes = [C.c_float]


# ---------------------------------------------------------------------------------------------------------------- the model
def idf_fix(total_structures, length):
    """-> (idf f32, its image in units of 2^-22)"""
    idf = np.float32(_libm.log2f(float(np.float32(total_structures) / np.float32(length))))
    v = float(idf)
    return idf, (int(v * 4194304.0 + 0.5) if 0.0 < v < 1.0e6 else 0)


def model_full(lists, rows, total_structures, penalty, first_id, n_structures):
    """lists: hash -> ascending absolute ids; rows: (hash[], node[], edge_j[]).  -> (REC array in ascending nid, per-structure integer sums of the
    listed structures, len per row, fix per row)"""
    qh, qn, qe = (np.asarray(a).astype(np.int64) for a in rows)
    match = np.zeros(n_structures, np.int64)
    sums = np.zeros(n_structures, np.uint64)
    lens = np.zeros(len(qh), np.int64)
    fixes = np.zeros(len(qh), np.uint64)
    by_node, by_edge = {}, {}
    for r in range(len(qh)):
        ids = lists.get(int(qh[r]))
        if ids is None or len(ids) == 0:
            continue
        lens[r] = len(ids)
        fix = idf_fix(total_structures, len(ids))[1]
        fixes[r] = fix
        loc = np.asarray(ids, np.int64) - first_id
        loc = loc[(loc >= 0) & (loc < n_structures)]
        match[loc] += 1
        sums[loc] += np.uint64(fix)
        by_node.setdefault(int(qn[r]), []).append(loc)
        by_edge.setdefault((int(qn[r]), int(qe[r])), []).append(loc)
    assert int(fixes.max(initial=0)) * max(len(qh), 1) < 1 << 63          # the uint64 sums are the exact integer sums
    nodes = np.zeros(n_structures, np.int64)
    edges = np.zeros(n_structures, np.int64)
    for groups, out in ((by_node, nodes), (by_edge, edges)):
        for parts in groups.values():
            out[np.unique(np.concatenate(parts))] += 1
    hit = np.flatnonzero(match > 0)
    rec = np.zeros(len(hit), REC)
    rec["nid"] = hit + first_id
    rec["total_match_count"] = match[hit]
    rec["node_count"] = nodes[hit]
    rec["edge_count"] = edges[hit]
    rec["idf"] = (sums[hit].astype(np.float64) / 4194304.0).astype(np.float32) * np.asarray(penalty, np.float32)[hit]
    return rec, [int(x) for x in sums[hit]], lens, fixes


def rank(full, top_n):
    key = full["idf"] + np.float32(0.0)          # -0 -> +0
    order = np.lexsort((full["nid"], -key))
    return full[order][:top_n]


def model_count(lists, rows, total_structures, penalty, first_id, n_structures, top_n):
    full = model_full(lists, rows, total_structures, penalty, first_id, n_structures)[0]
    return full if top_n == 0 else rank(full, top_n)


# ---------------------------------------------------------------------------------------------------------------- layout of a list, for the claims
def vlen(v):
    v = np.asarray(v, np.int64)
    return 1 + (v >= 1 << 7).astype(np.int64) + (v >= 1 << 14) + (v >= 1 << 21) + (v >= 1 << 28)


def varint_spans(ids_abs):
    """-> (first byte of every posting's varint inside the list, its width, bytes of the list)"""
    ids = np.asarray(ids_abs, np.int64)
    w = vlen(np.concatenate([ids[:1], np.diff(ids)]))
    end = np.cumsum(w)
    return end - w, w, int(end[-1])


def list_bytes(ids_abs):
    return varint_spans(ids_abs)[2]


def qt_stride(n_bytes, nc=NC):
    """checkpoint stride of a list: the smallest j with >= 48 bytes per chunk of 2^j cells -> (j, chunks)"""
    j = 0
    while True:
        ne = (nc + (1 << j) - 1) >> j
        if ne <= 1 or n_bytes >= 48 * ne:
            return j, max(ne, 1)
        j += 1


def pieces(ids_abs, first_id):
    """the byte ranges [lo, hi) the checkpoints cut a list into, one per chunk of 2^j cells: chunk e begins at the first varint whose id lies at or
    behind its first cell (ids below first_id belong to chunk 0, ids beyond the range to none)"""
    ids = np.asarray(ids_abs, np.int64)
    start, _, n = varint_spans(ids)
    j, ne = qt_stride(n)
    loc = ids - first_id
    ent = np.where(loc < 0, 0, np.where(loc >= S, ne, (np.maximum(loc, 0) >> CELL_LOG2) >> j))
    cut = [0] + [int(start[np.argmax(ent >= b)]) if (ent >= b).any() else n for b in range(1, ne)] + [n]
    return [(cut[e], cut[e + 1]) for e in range(ne)]


def slots_of(ids_abs, first_id):
    return [(hi - lo + 15) // 16 for lo, hi in pieces(ids_abs, first_id) if hi > lo]


def order_key(idf):
    b = int((np.float32(idf) + np.float32(0.0)).view(np.uint32))
    return (~b & 0xffffffff) if b & 0x80000000 else (b | 0x80000000)


K0 = 0xB7800000


def key_bin(key):
    return 0 if key < K0 else min(((key - K0) >> 17) + 1, 2047)


def sub_bin(key):
    b = key_bin(key)
    edge = K0 + ((b - 1) << 17) if b else 0
    return min((key - edge) >> (21 if b == 0 else 20 if b == 2047 else 6), 2047)


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    """lists: ids relative to first_id (np.int64, ascending); queries: per query (list index[], node[], edge_j[]) (batch) or names of maps (maps, with
    `slots`: the map's distinct-hash position of every list, None = a filler hash no map holds)"""

    def __init__(self, name, cls, lists, queries, penalty=None, total=4 * S, top_ns=(5, 100), claims=None, via="batch", slots=None, in_range=True):
        self.name, self.cls, self.lists, self.queries, self.total, self.top_ns, self.via = name, cls, lists, queries, total, tuple(top_ns), via
        self.penalty = default_penalty() if penalty is None else np.asarray(penalty, np.float32)
        self.claims = claims or {}
        self.slots = slots
        self.in_range = in_range          # every id inside [first_id, first_id + S): the index must verify clean
        self.base_queries = queries       # (a map variant: the batch query it restates, as list indices)

    def __repr__(self):
        return f"Case({self.cls}/{self.name}/{self.via})"

    def abs_lists(self, first_id):
        out = []
        for l in self.lists:
            a = np.asarray(l, np.int64) + first_id
            out.append(a[(a >= 0) & (a < 1 << 32)])
        return out

    def hashes(self, map_hashes=None):
        """the hash of every list: 3 k + 1 (batch), or the slot's hash of the map / a filler hash that no map holds (maps)"""
        if self.via == "batch":
            return [3 * k + 1 for k in range(len(self.lists))]
        held = set(int(h) for h in map_hashes)
        fill, out = 7, []
        for k in range(len(self.lists)):
            s = k if self.slots is None else self.slots[k]
            if s is not None:
                out.append(int(map_hashes[s]))
            else:
                while fill in held:
                    fill += 1
                out.append(fill)
                fill += 1
        return out

    def index(self, first_id, map_hashes=None):
        """-> (hashes u32[H], offsets u64[H + 1], value u8[], {hash: absolute ids}) — lists that keep no id are left out"""
        pairs = sorted((h, a) for h, a in zip(self.hashes(map_hashes), self.abs_lists(first_id)) if len(a))
        blobs = [encode([int(x) for x in a]) for _, a in pairs]
        off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
        return (np.array([h for h, _ in pairs], np.uint32), off, np.frombuffer(b"".join(blobs), np.uint8).copy(), {h: a for h, a in pairs})

    def rows(self, maps=None):
        """per query (hash[], node[], edge_j[])"""
        if self.via == "maps":
            return [tuple(np.asarray(a, np.uint32) for a in maps[m]) for m in self.queries]
        h = np.array(self.hashes(), np.uint32)
        return [(h[np.asarray(li, np.int64)], np.asarray(n, np.uint32), np.asarray(e, np.uint32)) for li, n, e in self.queries]


def default_penalty():
    i = np.arange(S, dtype=np.int64)
    return (1.0 / np.sqrt((50 + (i * 7919) % 900).astype(np.float64))).astype(np.float32)


def _ids(*parts):
    return np.unique(np.concatenate([np.asarray(p, np.int64).ravel() for p in parts]))


def fill_to_bytes(first_id, anchors, n_bytes, run_at=0):
    """the anchors plus a run of consecutive ids behind anchors[run_at], as long as it takes for the encoding to be exactly n_bytes"""
    anchors = np.asarray(anchors, np.int64)

    def make(k):
        return _ids(anchors, anchors[run_at] + 1 + np.arange(k))
    lo, hi = 0, n_bytes
    while lo < hi:          # the length grows by 0 or 1 per id added
        mid = (lo + hi) // 2
        if list_bytes(make(mid) + first_id) < n_bytes:
            lo = mid + 1
        else:
            hi = mid
    out = make(lo)
    assert list_bytes(out + first_id) == n_bytes, (first_id, n_bytes)
    return out


def _simple_query(n_lists, group=3):
    k = np.arange(n_lists)
    return (k, k // group, (k // 2) % 2)


ALL_TILES = np.array([5, 16384 + 7, 2 * 16384 + 9, 3 * 16384 + 11, 4 * 16384 + 13, 5 * 16384 + 100], np.int64)


def stride_cases(first_id):
    lists, want = [], []
    for t in STRIDE_THRESHOLDS:
        for n in (t - 1, t):
            lists.append(fill_to_bytes(first_id, ALL_TILES + 40 * len(lists), n))
            want.append(n)
    edge = Case("thresholds", "stride", lists, [_simple_query(len(lists))], claims=dict(bytes=want))
    dense = Case("dense", "stride", [np.arange(S, dtype=np.int64), ALL_TILES, fill_to_bytes(first_id, ALL_TILES + 1, 300)], [_simple_query(3)],
                 claims=dict(dense=0), top_ns=(5, 1000))
    # whole tiles without a posting: tiles 1, 2, 4, 5 empty (an entry per cell), only tile 2 used (nothing before, nothing behind), a short list
    # that ends in tile 0, and one whose last chunks are empty at a coarse stride
    gaps = [_ids(np.arange(100, 1300), 3 * 16384 + np.arange(50, 1250)), 2 * 16384 + 3000 + 2 * np.arange(1200), np.arange(7, 2300),
            fill_to_bytes(first_id, [9, 700, 5000], 200), _ids(4 * 16384 + np.arange(300))]
    empty = Case("empty_tiles", "stride", gaps, [_simple_query(len(gaps))],
                 claims=dict(empty_tiles=[[1, 2, 4, 5], [0, 1, 3, 4, 5], [1, 2, 3, 4, 5], [1, 2, 3, 4, 5], [0, 1, 2, 3, 5]]))
    at = [0, 2047, 2048, 16383, 16384, S - 1]
    ones = Case("one_posting", "stride", [np.array([x], np.int64) for x in at], [_simple_query(len(at), 1), (np.array([5]), np.array([0]), np.array([1]))],
                claims=dict(single=at), top_ns=(3,))
    return [edge, dense, empty, ones]


def _can_step_2_28(first_id):
    return first_id >= (1 << 28) - 40000 or first_id + S + (1 << 28) + 4000 < 1 << 32


def _run_of_bytes(first_id, head, n_bytes):
    """consecutive ids from `head` whose encoding at the start of a list takes n_bytes"""
    run = head + np.arange(n_bytes - int(vlen(first_id + head)) + 1)
    assert list_bytes(run + first_id) == n_bytes
    return run


def _straddle_list(first_id, block, before, width, mult):
    """a list in which a varint of `width` bytes begins `before` bytes ahead of byte mult * block.  block 64: counted from the list's first byte, the list has
    an entry per cell (>= 2112 bytes) and the varint is the first posting of a new cell.  block 16: counted from the first byte of the PIECE the
    checkpoints cut (a coarse stride: the varint stays inside its piece).  width 5: a step of 2^28 + x — from below first_id into the range where such ids
    exist, else from the range to beyond it.  -> (ids, every id in range)"""
    at = mult * block - before
    if width < 5:
        step = 200 if width == 2 else 20000
        if block == 64:          # one-byte deltas that end just below cell 1, the step into it (or behind it), then an entry per cell
            run = _run_of_bytes(first_id, 2040 - at, at)
            return _ids(run, run[-1] + step + np.arange(2300)), True
        run = _run_of_bytes(first_id, 100, at)          # 144 .. 287 bytes: chunks of 16 cells, the step stays in chunk 0
        return _ids(run, run[-1] + step + np.arange(120)), True
    if first_id >= (1 << 28) - 40000:          # the absolute ids 1 .. at (a byte each), then into the range
        lo = np.arange(1, at + 1) - first_id
        if block == 64:
            return _ids(lo, 41000 + np.arange(2300)), False
        return _ids(lo, 50000 + np.arange(60)), False          # 96 .. 143 bytes: two chunks of 32 cells, the step lands in chunk 0
    if block == 64:          # 64 * 36 - before bytes in cells 0 and 1, then beyond the range
        run = _run_of_bytes(first_id, 3, 64 * 36 - before)
        return _ids(run, run[-1] + (1 << 28) + 5 + np.arange(3)), False
    run = _run_of_bytes(first_id, 70000, at)          # fewer than 96 bytes: the list is one piece
    return _ids(run, run[-1] + (1 << 28) + 5 + np.arange(3)), False


def straddles(ids_abs, unit, first_id):
    """varints that straddle a multiple of `unit` bytes, relative to the piece they lie in (unit 16) or to the list (unit 64): (width, bytes before the
    boundary, the posting opens a new cell or leaves the range)"""
    ids = np.asarray(ids_abs, np.int64)
    start, w, _ = varint_spans(ids)
    base = np.zeros(len(ids), np.int64)
    if unit == 16:
        for lo, hi in pieces(ids, first_id):
            base[(start >= lo) & (start < hi)] = lo
    rel = start - base
    loc = ids - first_id
    cell = np.where(loc < 0, -1, np.where(loc >= S, NC, np.maximum(loc, 0) >> CELL_LOG2))
    newcell = np.concatenate([[False], cell[1:] > cell[:-1]])
    out = set()
    for k in np.flatnonzero((rel // unit) != ((rel + w - 1) // unit)):
        out.add((int(w[k]), int(unit - rel[k] % unit), bool(newcell[k])))
    return out


def carry_cases(first_id):
    lists, want, inr = [], [], True
    for width in (2, 3, 5):
        for before in range(1, width):
            for unit in (1, 2):
                if width == 5 and not _can_step_2_28(first_id):
                    continue
                ids, ok = _straddle_list(first_id, 64, before, width, unit)
                inr = inr and ok
                lists.append(ids)
                want.append((width, before))
    return [Case("block_carry", "carry", lists, [_simple_query(len(lists))], claims=dict(straddle64=want), in_range=inr, top_ns=(5, 2000))]


def slot_cases(first_id):
    rng = np.random.Generator(np.random.PCG64(SEED + 1))
    # cells of n one-byte postings: cell 1: 1023 (after a two-byte step: 1024 bytes = 64 slots), cell 3: 1024 (65 slots), cell 5: 1025, cells 7 + 8: the last
    # id of cell 7 and all of cell 8 (2048 bytes = 128 slots); + enough elsewhere for an entry per cell
    cells = _ids(np.arange(500), 2048 + np.arange(1023), 3 * 2048 + np.arange(1024), 5 * 2048 + np.arange(1025), [8 * 2048 - 1], 8 * 2048 + np.arange(2048),
                 20 * 2048 + 3 * np.arange(300))
    full = Case("cell_counts", "slots", [cells, ALL_TILES], [_simple_query(2)], claims=dict(slots=[64, 65, 128]), top_ns=(5, 3000))
    # single-piece lists (< 96 bytes) of 31 / 32 / 33 and 47 / 48 / 49 bytes whose last varint has 1, 2 and 3 bytes
    ends, want_end = [], []
    for n in (31, 32, 33, 47, 48, 49):
        for wl in (1, 2, 3):
            last = {1: 1, 2: 300, 3: 17000}[wl]
            body = fill_to_bytes(first_id, ALL_TILES[:3] + 50 * len(ends), n - wl)
            ends.append(_ids(body, [body[-1] + last]))
            want_end.append((n, wl))
    tails = Case("piece_ends", "slots", ends, [_simple_query(len(ends))], claims=dict(ends=want_end))
    # the look-back: varints of 2, 3 (and 5) bytes with 1 .. width - 1 bytes in the slot before
    lb, want_lb, inr = [], [], True
    for width in (2, 3, 5):
        for before in range(1, width):
            if width == 5 and not _can_step_2_28(first_id):
                continue
            ids, ok = _straddle_list(first_id, 16, before, width, 3)
            inr = inr and ok
            lb.append(ids)
            want_lb.append((width, before))
    look = Case("look_back", "slots", lb, [_simple_query(len(lb))], claims=dict(straddle16=want_lb), in_range=inr, top_ns=(5, 2000))
    # next-fit: 12 pieces of 5 slots, one of 3 / 4 / 5 (63 / 64 / 65 slots so far), then one of 2 slots; every list is one piece that every tile decodes
    win_lists, queries = [], []
    for q, third in enumerate((48, 64, 80)):
        first = len(win_lists)
        for n in [80] * 12 + [third, 32]:
            win_lists.append(fill_to_bytes(first_id, ALL_TILES + int(rng.integers(200, 1800)) + 3 * len(win_lists), n))
        k = np.arange(first, len(win_lists))
        queries.append((k, k - first, np.zeros(len(k), np.int64)))
    wins = Case("windows", "slots", win_lists, queries, claims=dict(window_sums=[63, 64, 65]))
    return [full, tails, look, wins]


def tie_cases(first_id):
    ones = np.ones(S, np.float32)
    runs = _ids(np.arange(16380, 16391), np.arange(32760, 32776))
    a = 100 + 7 * np.arange(10)
    b = _ids(40000 + 5 * np.arange(500), runs[::2])
    b = np.setdiff1d(b, runs)          # the runs' structures are hit by the same rows: T and T2 only
    t1 = Case("tile_edges", "ties", [a, runs, runs.copy(), b, a.copy()], [(np.arange(5), np.array([0, 1, 1, 2, 3]), np.array([1, 0, 0, 1, 1]))],
              penalty=ones, top_ns=(12, 15, 21, 22, 25, 30, 37, 38), claims=dict(tied=[len(runs)], above=10))
    n = 8
    run2 = _ids(16384 - n + np.arange(n), 16384 + np.arange(n + 1))
    t2 = Case("tile_topn", "ties", [run2, b], [(np.arange(2), np.array([0, 1]), np.array([1, 0]))], penalty=ones, top_ns=(n, n + 1, n + 2),
              claims=dict(tied=[len(run2)], above=0, per_tile=(n, n + 1)))
    return [t1, t2]


def crowd_cases(first_id):
    out = []
    eps = np.nextafter(np.float32(1.0), np.float32(2.0))
    bg = 37 + 27 * np.arange(3000)          # background structures: a longer list, a lower key in another bin
    for ulp in (False, True):
        for K in (1073, 1074, 1075):
            ties = 81 * np.arange(K)
            extra = 81 * K + 3          # one key a little lower, in the same first-level bin
            pen = np.ones(S, np.float32)
            pen[extra] = np.float32(1.0 - 2.0 ** -12)
            if ulp:
                pen[ties[1::2]] = eps
            # total_structures: a value for which the ties' key leaves room above it in its 64-key sub-bin and below it in its first-level bin
            total = 4 * S
            while True:
                k0 = order_key(np.float32(idf_fix(total, K + 1)[1] / 4194304.0))
                if (k0 & 63) <= 60 and ((k0 - K0) & 0x1ffff) >= 1 << 13:
                    break
                total += 1
            out.append(Case(f"ties{K}{'_ulp' if ulp else ''}", "crowd", [_ids(ties, [extra]), np.setdiff1d(bg, ties)], [_simple_query(2, 1)], penalty=pen,
                            total=total, top_ns=(50,), claims=dict(crowd=K, ulp=ulp, overflow=K > 1074)))
    hit = 11 * np.arange(3100)
    pen = np.zeros(S, np.float32)
    pen[hit[:30]] = 1.0 + 0.01 * np.arange(30)
    pen[hit[30:35]] = -0.0
    pen[hit[35:55]] = -1.0 - 0.5 * np.arange(20)
    out.append(Case("bin0", "crowd", [hit, hit[::3]], [_simple_query(2, 1)], penalty=pen, top_ns=(50,), claims=dict(cut_bin=0, zeros=3100 - 50)))
    hit2 = 13 * np.arange(2000)
    pen2 = default_penalty()
    pen2[hit2] = (1.0e5 * (1.0 + 1.0e-3 * np.arange(2000))).astype(np.float32)
    out.append(Case("bin2047", "crowd", [hit2, _ids(hit2[::2], 5 + 17 * np.arange(900))], [_simple_query(2, 1)], penalty=pen2, top_ns=(50,), claims=dict(cut_bin=2047)))
    return out


def width_cases(first_id, map_slots=True):
    """through query maps: list k on the map's k-th distinct hash"""
    X = 40000
    one = [np.array([X], np.int64) for _ in range(32)]
    l32768 = _ids(np.arange(10000, 10000 + 32768))
    l32768b = _ids(np.arange(35000, 35000 + 32768))
    l32769 = _ids(np.arange(30000, 30000 + 32769))
    assert X in l32768 and X in l32768b and X in l32769
    near = Case("near_wrap", "width", one + [l32768, l32769], ["big"], total=1 << 31, via="maps", claims=dict(sum_at=X, sum_lo=(1 << 32) - (1 << 12), sum_hi=1 << 32, sums32=True),
                top_ns=(5, 100))
    exact = Case("exact_wrap", "width", one + [l32768, l32768b], ["big"], total=1 << 31, via="maps", claims=dict(sum_at=X, sum_lo=1 << 32, sum_hi=(1 << 32) + 1, sums32=False),
                 top_ns=(5, 100))
    zero = Case("zero_units", "width", [np.arange(S, dtype=np.int64), 50 * np.arange(400), _ids(50 * np.arange(300) + 1, [70000])], ["big"], total=S, via="maps",
                claims=dict(zero_unit_row=0, only_zero=S - 400 - 301, sums32=False), top_ns=(5, 100))
    wide = Case("total_2_33", "width", [np.array([77], np.int64), 9 * np.arange(100), np.array([77, 5000], np.int64)], [_simple_query(3, 2)], total=1 << 33,
                claims=dict(packed=False, min_fix=1 << 27), top_ns=(5,))
    return [near, exact, zero, wide]


def kept_row_cases(first_id, small_slots):
    """128 / 129 kept rows of the 160-entry map (lists of ~500 postings: idf ~ 7.5, a query's units stay below 2^32 either way), and a batch of the big map
    between two small ones that keep 5 rows.  small_slots: the big map's slots of the small map's hashes"""
    rng = np.random.Generator(np.random.PCG64(SEED + 2))
    out = []

    def lists(n):
        return [np.sort(rng.choice(S, size=int(rng.integers(480, 520)), replace=False)).astype(np.int64) for _ in range(n)]
    for n in (128, 129):
        out.append(Case(f"kept{n}", "rows", lists(n), ["big"], total=S, via="maps", claims=dict(kept=[n], sums32=n <= 128), top_ns=(5, 100)))
    keep_small = list(small_slots[:5])
    others = [s for s in range(MAX_MAP_ROWS) if s not in set(small_slots)][:124]
    out.append(Case("mixed129", "rows", lists(129), ["small", "big", "small"], total=S, via="maps", slots=keep_small + others, claims=dict(kept=[5, 129, 5], sums32=False),
                    top_ns=(5, 100)))
    out.append(Case("mixed128", "rows", lists(128), ["small", "big", "small"], total=S, via="maps", slots=keep_small + others[:123], claims=dict(kept=[5, 128, 5], sums32=True),
                    top_ns=(5, 100)))
    return out


def many_row_cases(first_id):
    """1024 / 1025 rows and, as one query, 4095 / 4096 rows of a 4,200-list index of short lists; rows out of (node, edge) order"""
    rng = np.random.Generator(np.random.PCG64(SEED + 3))
    lists = [np.sort(rng.choice(S, size=int(rng.integers(2, 9)), replace=False)).astype(np.int64) for _ in range(4200)]
    lists[0] = _ids(lists[0], 16 * np.arange(5000))          # some longer ones: pieces in every cell
    lists[1] = np.arange(S, dtype=np.int64)[::2]
    out = []
    for n in (1024, 1025, 4095, 4096):
        k = rng.permutation(np.concatenate([[0, 1], 2 + rng.permutation(4198)[:n - 2]]))
        node, edge = rng.integers(0, 40, n), rng.integers(0, 3, n)
        out.append(Case(f"rows{n}", "rows", lists, [(k, node, edge)], claims=dict(kept=[n]), top_ns=(5, 100)))
    return out


def group_cases(first_id):
    rng = np.random.Generator(np.random.PCG64(SEED + 4))
    sizes = [31, 1, 1, 70, 1, 1, 1]
    while sum(sizes) < 1000:
        sizes.append(int(min(rng.integers(1, 6), 1000 - sum(sizes))))
    ends = np.cumsum(sizes) - 1
    gid = np.repeat(np.arange(len(sizes)), sizes)
    node, edge = gid // 3, gid % 3          # three edge groups per node
    universe = 64 * np.arange(1300) + 11
    lists = [np.sort(rng.choice(universe, size=int(rng.integers(3, 7)), replace=False)).astype(np.int64) for _ in range(1000)]
    X1, X2, X3 = 64 * 1300 + 100, 64 * 1300 + 101, 64 * 1300 + 102          # hit by non-end rows of group 0 only, by its end row only, by one row of every group
    lists[0] = _ids(lists[0], [X1])
    lists[5] = _ids(lists[5], [X1])
    lists[30] = _ids(lists[30], [X2])
    for g, e in enumerate(ends):
        r = int(e - rng.integers(0, sizes[g]))
        lists[r] = _ids(lists[r], [X3])
    perm = rng.permutation(1000)          # out of (node, edge) order; the rows of a group keep their order among themselves (the host's sort is stable)
    for g in range(len(sizes)):
        at = np.flatnonzero(gid[perm] == g)
        perm[at] = np.sort(perm[at])
    q1 = (perm, node[perm], edge[perm])
    q2 = (np.arange(0, 1000, 7), np.zeros(143, np.int64), np.zeros(143, np.int64))          # all rows on one node, one edge
    q3 = (np.arange(100), np.arange(100), np.zeros(100, np.int64))                            # single-row groups only
    return [Case("word_edges", "groups", lists, [q1, q2, q3], claims=dict(group_ends=[30, 31, 32], span=(33, 102), X=(X1, X2, X3), n_groups=len(sizes)), top_ns=(5, 100))]


def shard_cases(first_id):
    lists = [_ids(np.arange(-50, 40), np.arange(S - 30, S + 51)), _ids(-3000 + 7 * np.arange(400), [16384]), _ids(S - 1 + np.arange(300) * 3),
             _ids(np.arange(-2500, -2400)), _ids(S + np.arange(5, 90)), _ids(np.arange(-5, 5), 2048 * np.arange(1, 43), np.arange(S - 2, S + 3)),
             fill_to_bytes(first_id, ALL_TILES, 2200)]
    return [Case("edges", "shard", lists, [_simple_query(len(lists))], in_range=False, claims=dict(outside=[3, 4]))]


def batch_cases(first_id):
    return (stride_cases(first_id) + carry_cases(first_id) + slot_cases(first_id) + tie_cases(first_id) + crowd_cases(first_id) + width_cases(first_id)[3:]
            + many_row_cases(first_id) + group_cases(first_id) + shard_cases(first_id))


def map_variants(cases):
    """every query of at most MAX_MAP_ROWS distinct lists of a batch case as a map case of its own: its lists on the map's first hashes, every other list
    of the case on filler hashes"""
    out = []
    for c in cases:
        if c.via != "batch":
            continue
        for qn, (li, _, _) in enumerate(c.queries):
            li = [int(x) for x in li]
            if len(li) > MAX_MAP_ROWS or len(set(li)) != len(li):
                continue
            pos = {k: s for s, k in enumerate(li)}
            claims = dict(c.claims)
            if "window_sums" in claims:
                claims["window_sums"] = [claims["window_sums"][qn]]
            out.append(Case(f"{c.name}_q{qn}", c.cls, c.lists, ["big"], penalty=c.penalty, total=c.total, top_ns=c.top_ns, claims=claims, via="maps",
                            slots=[pos.get(k) for k in range(len(c.lists))], in_range=c.in_range))
            out[-1].base_queries = [c.queries[qn]]
    return out


def map_slots(big_hash, small_hash):
    """-> (the big map's distinct hashes in order of first appearance, the positions among them of the small map's hashes)"""
    big = [int(h) for h in big_hash]
    distinct = sorted(set(big), key=big.index)
    assert len(distinct) >= MAX_MAP_ROWS
    return np.array(distinct, np.uint32), [distinct.index(int(h)) for h in sorted(set(int(x) for x in small_hash), key=[int(x) for x in small_hash].index)]


def map_cases(first_id, small_slots):
    b = [c for c in batch_cases(first_id) if c.cls not in ("rows", "groups") and c.name != "total_2_33"]
    return width_cases(first_id)[:3] + kept_row_cases(first_id, small_slots) + map_variants(b)
