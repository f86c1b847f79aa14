"""Sorted (hash, id) streams for the posting encoder (csrc/k_index.hip) and a plain numpy model of the index it must write.  Shared by
tests/test_encoder_cases_host.py (model == oracle, every claimed property asserted on the model) and tests/test_gpu_encoder_edges.py (device == model,
byte for byte).  Not a test module.

The encoder works on tiles of TILE = 2,048 stream elements: 256 threads own ITEMS = 8 consecutive elements each, 64 threads are a wavefront (512
elements).  Stream element p is item p % 8 of thread p // 8 % 256; an element that repeats its predecessor writes nothing."""
import numpy as np

ITEMS, WAVE, TILE = 8, 512, 2048
BOUNDARY_VALUES = (0x7f, 0x80, 0x3fff, 0x4000, 0x1fffff, 0x200000, 0xfffffff, 0x10000000, 0xffffffff)
# where a boundary value is placed.  A: each of a thread's eight item positions (in eight different threads), the last item of a wavefront and of
# a tile; B: the first item of the next wavefront and of the next tile (a delta needs its predecessor, so neighbours go to different streams)
POSITIONS_A = tuple(8 * (3 + 2 * j) + j for j in range(ITEMS)) + (WAVE - 1, TILE - 1)
POSITIONS_B = (WAVE, TILE)


def varint_len(v):
    v = np.asarray(v, np.uint64)
    return (1 + (v >= 1 << 7) + (v >= 1 << 14) + (v >= 1 << 21) + (v >= 1 << 28)).astype(np.int64)


class Model:
    """the index of a sorted stream: value, hashes, offsets, last_ids, n_postings — and per stream element what the encoder's classifier sees
    (item_len: bytes written, 0 for a repeat; item_head; item_delta: the value written)"""

    def __init__(self, hashes, ids):
        h = np.asarray(hashes, np.uint32)
        i = np.asarray(ids, np.uint32)
        n = len(h)
        assert len(i) == n
        key = (h.astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
        assert np.all(key[1:] >= key[:-1]), "stream not sorted by (hash, id)"
        first = np.ones(n, bool)
        first[1:] = False
        keep = first | np.concatenate([[True], key[1:] != key[:-1]])[:n]
        head = first | np.concatenate([[True], h[1:] != h[:-1]])[:n]
        prev = np.concatenate([[0], i[:-1]]).astype(np.int64)[:n]
        delta = np.where(head, i.astype(np.int64), i.astype(np.int64) - prev).astype(np.uint64)
        ln = np.where(keep, varint_len(delta), 0)
        self.item_len, self.item_head, self.item_delta = ln, head & keep, np.where(keep, delta, 0)
        kd, kl = delta[keep], ln[keep]
        start = np.concatenate([[0], np.cumsum(kl)]).astype(np.int64)
        value = np.zeros(int(start[-1]), np.uint8)
        for b in range(5):
            m = kl > b
            byte = ((kd[m] >> np.uint64(7 * b)) & np.uint64(0x7f)).astype(np.uint8) | np.where(kl[m] > b + 1, 0x80, 0).astype(np.uint8)
            value[start[:-1][m] + b] = byte
        kh = head[keep]
        self.value = value
        self.hashes = h[keep][kh]
        self.offsets = np.concatenate([start[:-1][kh], [start[-1]]]).astype(np.uint64)
        ki = i[keep]
        last = np.concatenate([kh[1:], [True]])[:len(ki)] if len(ki) else np.zeros(0, bool)
        self.last_ids = ki[last]
        self.n_postings = int(keep.sum())
        self.n_structures = int(i.max()) + 1 if n else 0


def _filler(rng, n, hash0, max_delta=300, n_lists=None):
    """n elements of ordinary lists (hashes ascending from hash0, a few elements per list, small deltas, now and then a repeat) -> (h, id)"""
    n_lists = max(1, n // 9) if n_lists is None else n_lists
    h = hash0 + np.sort(rng.integers(0, n_lists, n)).astype(np.int64) * 3
    step = rng.integers(0, max_delta, n)
    step[rng.random(n) < 0.1] = 0
    ids = np.zeros(n, np.int64)
    run = 0
    for p in range(n):
        run = step[p] if p == 0 or h[p] != h[p - 1] else run + step[p]
        ids[p] = run
    return h.astype(np.uint32), ids.astype(np.uint32)


def sizes_case(n, seed=11):
    rng = np.random.default_rng(seed + n)
    return _filler(rng, n, 1000)


def boundary_case(value, kind, positions, seed=23):
    """a stream of just over a tile in which the element at every p of `positions` writes `value`: as the absolute id of a list head
    (kind "head") or as the delta to its predecessor, a head of id 0 (kind "delta")"""
    rng = np.random.default_rng(seed)
    n = max(positions) + 40
    h, ids = _filler(rng, n, 0, max_delta=100)
    h = h.astype(np.int64) * 4                               # room for the special hashes between the filler's
    ids = ids.astype(np.int64)
    order_fix = np.zeros(n, np.int64)
    for p in positions:
        if kind == "head":
            order_fix[p] = 1
            ids[p] = value
        else:
            order_fix[p - 1] = 1
            ids[p - 1] = 0
            order_fix[p] = 1
            ids[p] = value
    # special elements get hashes of their own, ascending with the position: cumulative offsets keep the stream sorted
    bump = np.zeros(n, np.int64)
    for p in positions:
        q = p if kind == "head" else p - 1
        bump[q:] += 2                                        # a new hash starts at q ...
        bump[p + 1:] += 2                                    # ... and the filler behind p starts another one
    h = np.maximum.accumulate(h) + bump
    if kind == "delta":
        for p in positions:
            h[p] = h[p - 1]
    # the filler element behind a special one must be a head (its id is below the special id): guaranteed by the bump
    return h.astype(np.uint32), ids.astype(np.uint32)


def alignment_case(k, second="mixed", seed=31):
    """tile 0: one list of 2,016 + k one-byte postings and 32 - k repeats of its last id, so tile 1 starts at byte offset k mod 16;
    tile 1: 2,048 elements of new hashes ("mixed": ordinary lists; "heads": 2,048 distinct hashes; "five": 2,048 heads of five bytes) and a short tail"""
    assert 0 <= k < 16
    rng = np.random.default_rng(seed + k)
    m = 2016 + k
    h0 = np.zeros(TILE, np.int64) + 5
    i0 = np.concatenate([np.arange(m), np.full(TILE - m, m - 1)])
    if second == "mixed":
        h1, i1 = _filler(rng, TILE + 70, 100)
    elif second == "heads":
        h1 = 100 + np.arange(TILE + 70) * 2
        i1 = rng.integers(0, 1 << 32, TILE + 70)
    else:
        h1 = 100 + np.arange(TILE + 70) * 2
        i1 = rng.integers(1 << 28, 1 << 32, TILE + 70)
    return np.concatenate([h0, h1]).astype(np.uint32), np.concatenate([i0, i1]).astype(np.uint32)


def long_list_case(seed=41):
    """one list over three tiles, then two short ones"""
    rng = np.random.default_rng(seed)
    i0 = np.cumsum(rng.integers(1, 300, 2 * TILE + 900))
    h = np.concatenate([np.full(len(i0), 77), [78, 78, 90]])
    return h.astype(np.uint32), np.concatenate([i0, [5, 6, 0]]).astype(np.uint32)


def duplicate_case(tail, seed=43):
    """repeats across a thread boundary (elements 6..9), a wavefront boundary (510..513) and a tile boundary (2046..2049); tile 1 from element
    2,050 on repeats element 2,049 to its end, and tile 2 is `tail` more elements: 0 (the stream ends inside the run), or a few that go on"""
    rng = np.random.default_rng(seed)
    h, ids = _filler(rng, TILE + 2, 10, n_lists=150)
    h, ids = h.astype(np.int64), ids.astype(np.int64)
    for a, b in ((6, 9), (510, 513), (2046, 2049)):
        h[a:b + 1] = h[a]
        ids[a:b + 1] = ids[a]
        # keep the list behind the run sorted: the elements of the same hash behind it restart from the run's id
        p = b + 1
        while p < len(h) and h[p] == h[a]:
            ids[p] = max(ids[p], ids[a])
            p += 1
    # make sure every list is ascending after the edits
    for p in range(1, len(h)):
        if h[p] == h[p - 1] and ids[p] < ids[p - 1]:
            ids[p] = ids[p - 1]
    run_h, run_i = h[-1], ids[-1]
    h = np.concatenate([h, np.full(2 * TILE - len(h), run_h)])
    ids = np.concatenate([ids, np.full(len(h) - len(ids), run_i)])
    if tail:
        h = np.concatenate([h, np.full(tail, run_h)])
        ids = np.concatenate([ids, np.concatenate([[run_i], run_i + 1 + np.arange(tail - 1) * 200])])
    return h.astype(np.uint32), ids.astype(np.uint32)


def all_cases():
    """name -> (hashes, ids, check) where check(model) asserts what the case is there for"""
    out = {}

    def add(name, hi, check):
        assert name not in out
        out[name] = (hi[0], hi[1], check)

    for n in (1, 2, 2047, 2048, 2049, 4097):
        def chk(m, n=n):
            assert len(m.item_len) == n and m.n_postings >= max(1, n // 2) and (m.item_len == 0).sum() >= (n > 100)
        add(f"n={n}", sizes_case(n), chk)
    for v in BOUNDARY_VALUES:
        for kind in ("head", "delta"):
            for tag, pos in (("A", POSITIONS_A), ("B", POSITIONS_B)):
                def chk(m, v=v, kind=kind, pos=pos):
                    want_len = int(varint_len(v))
                    for p in pos:
                        assert int(m.item_delta[p]) == v and int(m.item_len[p]) == want_len and bool(m.item_head[p]) == (kind == "head"), (hex(v), kind, p)
                    if pos is POSITIONS_A:
                        assert sorted(p % ITEMS for p in pos[:ITEMS]) == list(range(ITEMS)) and len({p // ITEMS for p in pos[:ITEMS]}) == ITEMS
                        assert pos[ITEMS] % WAVE == WAVE - 1 and pos[ITEMS + 1] % TILE == TILE - 1
                    else:
                        assert pos[0] % WAVE == 0 and pos[0] % TILE != 0 and pos[1] % TILE == 0
                add(f"{kind} {v:#x} {tag}", boundary_case(v, kind, pos), chk)
    for k in range(16):
        def chk(m, k=k):
            assert m.item_head[TILE] and int(m.offsets[1]) % 16 == k and int(m.item_len[:TILE].sum()) == int(m.offsets[1])
        add(f"tile 1 at byte {k} mod 16", alignment_case(k), chk)

    def chk_heads(m):
        assert m.item_head[TILE:2 * TILE].all() and int(m.offsets[1]) % 16 == 3
    add("2048 heads", alignment_case(3, "heads"), chk_heads)

    def chk_five(m):
        assert (m.item_len[TILE:2 * TILE] == 5).all() and int(m.offsets[1]) % 16 == 15      # 10,240 bytes behind the largest shift: LDS full
    add("2048 five-byte varints", alignment_case(15, "five"), chk_five)

    def chk_long(m):
        assert int(m.offsets[1]) == int(m.item_len[:2 * TILE + 900].sum()) and not m.item_head[1:2 * TILE + 900].any() and len(m.hashes) == 3
    add("one list over three tiles", long_list_case(), chk_long)
    for tail in (0, 5):
        def chk(m, tail=tail):
            for a, b in ((6, 9), (510, 513), (2046, 2049)):
                assert (m.item_len[a + 1:b + 1] == 0).all() and m.item_len[a] > 0
            assert (m.item_len[2050:2 * TILE] == 0).all() and not m.item_head[2050:2 * TILE].any()      # the tail of tile 1: 0 bytes, 0 heads
            assert len(m.item_len) == 2 * TILE + tail
            if tail:
                assert m.item_len[2 * TILE] == 0 and (m.item_len[2 * TILE + 1:] > 0).all()
        add(f"duplicate runs, tail {tail}", duplicate_case(tail), chk)

    def chk_only_dups(m):
        assert (m.item_len[TILE:2 * TILE] == 0).all() and not m.item_head[TILE:2 * TILE].any() and m.item_len[TILE - 1] > 0 and m.item_len[2 * TILE] > 0
    rng = np.random.default_rng(47)
    h, i = _filler(rng, TILE, 10)
    h2 = np.concatenate([h, np.full(TILE, h[-1]), [h[-1], h[-1] + 1]]).astype(np.uint32)
    i2 = np.concatenate([i, np.full(TILE, i[-1]), [int(i[-1]) + 70000, 3]]).astype(np.uint32)
    add("a tile of repeats of the previous tile's last element", (h2, i2), chk_only_dups)
    return out


def per_structure_lists(hashes, ids):
    """the stream as the oracle's input: per-structure sorted-unique hash lists in CSR form (structure = id)"""
    S = int(np.max(ids)) + 1
    pairs = np.unique((np.asarray(ids, np.uint64) << np.uint64(32)) | np.asarray(hashes, np.uint64))
    sid = (pairs >> np.uint64(32)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.bincount(sid, minlength=S))]).astype(np.uint64)
    return (pairs & np.uint64(0xffffffff)).astype(np.uint32), off
