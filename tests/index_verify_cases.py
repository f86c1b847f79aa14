"""Inputs of the index verification tests (test_index_verify_host.py, test_gpu_index_verify.py): a plain Python checker written from the table
of csrc/fd_verify.h (the yardstick: it shares no code with the library), hand-encoded clean indices, directed damage (one fixture per class,
placed where the device walk changes shape) and seeded random damage.

A case is a dict: name, value, hashes, offsets, n_structures, first_id, and expect = None (clean) or (class, slot)."""
import numpy as np

CLASSES = ("OFFSET_ENDS", "OFFSET_ORDER", "HASH_ORDER", "LIST_END", "VARINT_LONG", "VARINT_FORM", "ZERO_DELTA", "ID_RANGE")
SUM_CAP = 1 << 40


def bit(c):
    return 1 << (c - 1)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def py_list(b, first_id, limit):
    """one list (bytes) -> (mask of classes 4-8, terminator bytes, last id)"""
    mask = 0
    if b[-1] & 0x80:
        mask |= bit(4)
    runs, cur = [], []
    for x in b:
        cur.append(int(x))
        if x < 0x80:
            runs.append(cur)
            cur = []
    n_post = len(runs)
    if cur:
        runs.append(cur)              # the bytes of a varint that runs across the end of the list
    vals = []
    for r in runs:
        if len(r) > 5 or (len(r) == 5 and r[4] > 0x0f):
            mask |= bit(5)
        if len(r) > 1 and r[-1] == 0x00:
            mask |= bit(6)
        vals.append(sum((x & 0x7f) << (7 * min(i, 4)) for i, x in enumerate(r)))
    if any(v == 0 for v, r in zip(vals[1:], runs[1:]) if r[-1] < 0x80):
        mask |= bit(7)
    last = min(sum(vals), SUM_CAP)
    if vals[0] < first_id or last >= limit:
        mask |= bit(8)
    if mask & (bit(4) | bit(5)):
        mask &= ~(bit(6) | bit(7) | bit(8))
    return mask, n_post, last


def py_table(hashes, offsets, value_len):
    """-> {slot: mask of classes 1-3} of the bad slots"""
    H = len(hashes)
    bad = {}
    if int(offsets[0]) != 0:
        bad[0] = bad.get(0, 0) | bit(1)
    if int(offsets[H]) != value_len:
        bad[H] = bad.get(H, 0) | bit(1)
    o0, o1 = offsets[:-1], offsets[1:]
    for k in np.nonzero(~((o0 < o1) & (o1 <= np.uint64(value_len))))[0]:
        bad[int(k)] = bad.get(int(k), 0) | bit(2)
    for k in np.nonzero(~(hashes[:-1] < hashes[1:]))[0]:
        bad[int(k)] = bad.get(int(k), 0) | bit(3)
    return bad


def id_limit(first_id, n_structures):
    return min(first_id + n_structures, 1 << 32)


def report_of(bad, hashes, offsets, list_stage, totals=None):
    """the report as a plain dict, from {slot: mask} (and the totals of a clean index)"""
    H = len(hashes)
    r = dict(ok=not bad, n_bad=len(bad), counts={n: sum(1 for m in bad.values() if m & bit(c + 1)) for c, n in enumerate(CLASSES)},
             list_stage=list_stage, first_slot=None, first_hash=None, first_offset=None, first_classes=(), n_lists=0, n_postings=0, max_id=0,
             max_list_bytes=0)
    if bad:
        k = min(bad)
        r.update(first_slot=k, first_hash=int(hashes[k]) if k < H else 0, first_offset=int(offsets[k]),
                 first_classes=tuple(n for c, n in enumerate(CLASSES) if bad[k] & bit(c + 1)))
    else:
        r.update(totals)
    return r


def py_verify(value, hashes, offsets, n_structures, first_id=0, only=None, base=None):
    """the whole check.  only / base: re-check only the lists `only` of an index whose other lists are those of a clean index with the
    per-list arrays base = (terminators, last ids) (seeded damage on a large index)"""
    H = len(hashes)
    bad = py_table(hashes, offsets, len(value))
    if bad:
        return report_of(bad, hashes, offsets, False)
    limit = id_limit(first_id, n_structures)
    if base is None:
        post, last = np.zeros(H, np.int64), np.zeros(H, np.int64)
        ks = range(H)
    else:
        post, last = base[0].copy(), base[1].copy()
        ks = only
    for k in ks:
        m, post[k], last[k] = py_list(value[int(offsets[k]): int(offsets[k + 1])], first_id, limit)
        if m:
            bad[k] = m
    totals = dict(n_lists=H, n_postings=int(post.sum()), max_id=int(last.max()) if H else 0,
                  max_list_bytes=int(np.diff(offsets.astype(np.int64)).max()) if H else 0)
    return report_of(bad, hashes, offsets, True, totals)


def np_list_arrays(value, offsets):
    """(terminators, last ids) per list of a CLEAN index, vectorised (the seeded cases on the synthetic index start from it)"""
    term = value < 0x80
    idx = np.arange(len(value), dtype=np.int64)
    prev_term = np.maximum.accumulate(np.where(term, idx, -1))
    starts = offsets[:-1].astype(np.int64)
    before = np.concatenate([[-1], prev_term[:-1]])            # last terminator strictly before each byte
    pin = idx - before - 1
    contrib = (value & 0x7f).astype(np.int64) << (7 * np.minimum(pin, 4))
    return np.add.reduceat(term.astype(np.int64), starts), np.add.reduceat(contrib, starts)


def report_dict(r):
    """a library VerifyReport as the same plain dict"""
    return dict(ok=r.ok, n_bad=r.n_bad, counts=dict(r.counts), list_stage=r.list_stage, first_slot=r.first_slot, first_hash=r.first_hash,
                first_offset=r.first_offset, first_classes=tuple(r.first_classes), n_lists=r.n_lists, n_postings=r.n_postings, max_id=r.max_id,
                max_list_bytes=r.max_list_bytes)


# ---- hand-encoded indices --------------------------------------------------------------------------------------------------------
def varint(v):
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def encode_ids(ids):
    out, prev = bytearray(), None
    for i in ids:
        out += varint(i if prev is None else i - prev)
        prev = i
    return bytes(out)


def assemble(lists, hashes=None):
    """raw lists (bytes) -> (value, hashes, offsets)"""
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in lists], dtype=np.uint64)
    value = np.frombuffer(b"".join(lists), np.uint8).copy()
    h = np.arange(len(lists), dtype=np.uint32) * 977 + 13 if hashes is None else np.asarray(hashes, np.uint32)
    return value, h, off


def run_of_ones(first, n):
    """n bytes: the id `first` (one byte, < 128) and n - 1 deltas of 1"""
    return bytes([first]) + b"\x01" * (n - 1)


def clean_lists(shift=0):
    """lists that hold 1-, 2-, 3-, 4- and 5-byte varints, id 0 as a first id (shift = 0), one posting, every shape the device walk has
    (<= 8 bytes, <= 128, below and above 16 KiB) and their edges, and a list beyond 64 KiB"""
    long_ids = np.cumsum(np.tile([1, 130, 1, 17000, 1], 12000))                # 60,000 postings, 96,000 bytes
    ids = [[0], [5, 6, 200, 20200, 3020200, 0x20000000 + 3020200], [0xF0000000, 0xF0000001], long_ids.tolist(), [7], [300], range(1, 41),
           range(2, 3002, 3), range(1, 9), range(9, 9 + 128), range(9, 9 + 129), range(3, 3 + 16383), range(3, 3 + 16384), range(3, 3 + 16385),
           [0xFFFFF000]]
    return [encode_ids([i + shift for i in l]) for l in ids]


def clean_cases():
    v, h, o = assemble(clean_lists())
    yield dict(name="hand", value=v, hashes=h, offsets=o, n_structures=0xFFFFFFFF, first_id=0, expect=None)
    v, h, o = assemble(clean_lists(1000))
    yield dict(name="hand_shard", value=v, hashes=h, offsets=o, n_structures=0xFFFFFFFF - 1000, first_id=1000, expect=None)
    yield dict(name="empty", value=np.zeros(0, np.uint8), hashes=np.zeros(0, np.uint32), offsets=np.zeros(1, np.uint64), n_structures=0, first_id=0,
               expect=None)
    v, h, o = assemble([b"\x00"])
    yield dict(name="one_list", value=v, hashes=h, offsets=o, n_structures=1, first_id=0, expect=None)


# ---- directed damage ----------------------------------------------------------------------------------------------------------------
S_DIRECTED = 1_000_000      # structures of the directed index: every clean id is far below


def _base_lists(first=0):
    """small clean lists around the damaged one; ids first + 3 .."""
    f = first
    return [encode_ids([f + 3, f + 4]), encode_ids([f + 5]), encode_ids(range(f + 10, f + 400, 3)), encode_ids([f + 9, f + 300, f + 70000]), encode_ids([f + 8, f + 9])]


def _damaged_list(n, pos, dmg, first_byte=3):
    """a list of n clean bytes (first id first_byte, then deltas of 1) with the bytes dmg put in at byte pos (pos >= 1)"""
    assert 1 <= pos <= n - len(dmg)
    return bytes([first_byte]) + b"\x01" * (pos - 1) + dmg + b"\x01" * (n - pos - len(dmg))


# class -> the bytes that show exactly that class when they stand for clean varints inside a list (not at its head)
BYTE_DAMAGE = {
    "c5_six_bytes": (5, b"\x81\x80\x80\x80\x80\x01"),
    "c5_fifth_0x10": (5, b"\x80\x80\x80\x80\x10"),
    "c6_delta": (6, b"\x81\x00"),
    "c6_three": (6, b"\x81\x80\x00"),
    "c7_zero": (7, b"\x00"),
}
# list length -> byte positions of the damage: the edges of the walk's steps (64-byte and 256-byte windows, 32 bytes for the groups of eight
# lanes, 4 bytes per lane) and varints that straddle them
PLACES = {7: [1, 2], 100: [3, 4, 29, 30, 31, 32, 33, 63, 64, 65], 1000: [61, 62, 63, 64, 65, 251, 252, 253, 254, 255, 256, 257, 509, 511],
          70000: [63, 64, 65, 253, 254, 255, 256, 257, 16383, 16384, 65535, 69990]}


def directed_cases():
    base = _base_lists()
    H = len(base) + 1

    def case(name, lists, cls, slot, n=S_DIRECTED, first_id=0, hashes=None, tweak=None):
        v, h, o = assemble(lists, hashes)
        if tweak:
            v, h, o = tweak(v, h, o)
        return dict(name=name, value=v, hashes=h, offsets=o, n_structures=n, first_id=first_id, expect=(cls, slot))

    # classes 1-3 on the clean directed index
    clean = base + [encode_ids([20, 21])]
    yield case("c1_value_longer_than_last_offset", clean, 1, H, tweak=lambda v, h, o: (np.append(v, np.uint8(1)), h, o))
    yield case("c1_first_offset_not_zero", clean, 1, 0, tweak=lambda v, h, o: (v, h, np.concatenate([[np.uint64(1)], o[1:]])))
    for k in (0, 2, H - 1):
        def empty(v, h, o, k=k):
            o = o.copy()
            if k == H - 1:
                o[k] = o[k + 1]          # the last list empty (offsets[H] must stay)
                return v, h, o
            o[k + 1] = o[k]
            return v, h, o
        yield case(f"c2_empty_slot{k}", clean, 2, k if k < H - 1 else H - 1, tweak=empty)
    def reversed_(v, h, o):
        o = o.copy()
        o[3] = o[2] - np.uint64(1)
        return v, h, o
    yield case("c2_reversed_slot2", clean, 2, 2, tweak=reversed_)
    for k in (0, 2, H - 2):
        def same(v, h, o, k=k):
            h = h.copy()
            h[k] = h[k + 1]
            return v, h, o
        yield case(f"c3_equal_slot{k}", clean, 3, k, tweak=same)
    def swap(v, h, o):
        h = h.copy()
        h[3] = h[4] + 5
        return v, h, o
    yield case("c3_descending_slot3", clean, 3, 3, tweak=swap)
    # classes 4-7: in the first slot, the last slot, and inside lists of every walk shape at the edges of its steps
    for slot_name, at in (("first", 0), ("last", len(base)), ("mid", 2)):
        def put(lst, at=at):
            l = list(base)
            l.insert(at, lst)
            return l
        yield case(f"c4_{slot_name}_short", put(b"\x83"), 4, at)
        yield case(f"c4_{slot_name}_two", put(b"\x03\x81"), 4, at)
        for nm, (cls, dmg) in BYTE_DAMAGE.items():
            yield case(f"{nm}_{slot_name}", put(_damaged_list(12, 2, dmg)), cls, at)
    for n, places in PLACES.items():
        yield case(f"c4_len{n}", base[:2] + [_damaged_list(n, n - 1, b"\x81")] + base[2:], 4, 2)
        yield case(f"c4_len{n}_open_varint", base[:2] + [_damaged_list(n, n - 3, b"\x81\x80\x80")] + base[2:], 4, 2)
        for nm, (cls, dmg) in BYTE_DAMAGE.items():
            for pos in places:
                if pos + len(dmg) <= n:
                    yield case(f"{nm}_len{n}_at{pos}", base[:2] + [_damaged_list(n, pos, dmg)] + base[2:], cls, 2)
    # a clean varint of every length across the same edges must stay clean
    for n, places in PLACES.items():
        for pos in places:
            for good in (b"\x81\x01", b"\x81\x80\x01", b"\x81\x80\x80\x01", b"\x81\x80\x80\x80\x01"):
                if pos + len(good) <= n:
                    c = case(f"clean_len{n}_at{pos}_{len(good)}", base[:2] + [_damaged_list(n, pos, good)] + base[2:], 0, 0, n=0xFFFFFFFF)
                    c["expect"] = None
                    yield c
    # a first varint that is not canonical (class 6 only: class 7 does not apply to the head), a head of five bytes
    yield case("c6_head", base[:1] + [b"\x85\x00\x01"] + base[1:], 6, 1)
    yield case("c5_head_six_bytes", base[:1] + [b"\x85\x80\x80\x80\x80\x01\x01"] + base[1:], 5, 1)
    yield case("c5_head_fifth_0x10", base[:1] + [b"\x85\x80\x80\x80\x10\x01"] + base[1:], 5, 1)
    yield case("c6_c7_zero_in_two_bytes", base[:1] + [b"\x05\x80\x00\x01"] + base[1:], (6, 7), 1)
    # class 8
    yield case("c8_last_id_at_limit", base + [encode_ids([17, S_DIRECTED])], 8, len(base))
    yield case("c8_single_id_at_limit", [encode_ids([S_DIRECTED])] + base, 8, 0)
    yield case("c8_long_list_runs_over", base[:2] + [_damaged_list(70000, 65000, varint(S_DIRECTED))] + base[2:], 8, 2)
    yield case("c8_sum_wraps_32_bits", base[:2] + [b"\x03" + b"\xff\xff\xff\xff\x0f" * 3] + base[2:], 8, 2)
    shard = _base_lists(1000)
    yield case("c8_below_first_id", shard[:3] + [encode_ids([999, 1200])] + shard[3:], 8, 3, first_id=1000)
    yield case("c8_shard_id_at_limit", shard + [encode_ids([1001, 1000 + S_DIRECTED])], 8, len(shard), first_id=1000)
    c = case("shard_last_id_below_limit", shard + [encode_ids([1000, 999 + S_DIRECTED])], 0, 0, first_id=1000)
    c["expect"] = None
    yield c


# ---- seeded damage ---------------------------------------------------------------------------------------------------------------
def seeded_cases(value, hashes, offsets, seed, n_value, n_table):
    """single replacements IN PLACE (undone after each yield): n_value bytes of value, n_table entries each of offsets and hashes.
    yields (kind, position, lists whose bytes changed)"""
    rng = np.random.default_rng(seed)
    H = len(hashes)
    for _ in range(n_value):
        p = int(rng.integers(len(value)))
        old = int(value[p])
        new = old
        while new == old:
            new = int(rng.integers(256))
        value[p] = new
        k = int(np.searchsorted(offsets, p, side="right")) - 1
        yield "value", p, [k]
        value[p] = old
    for _ in range(n_table):
        k = int(rng.integers(H + 1))
        old = int(offsets[k])
        near = int(rng.integers(2))          # half of them near the old value (a slip of a few bytes), half anywhere up to twice the file
        new = old
        while new == old:
            new = max(0, old + int(rng.integers(-3, 4))) if near else int(rng.integers(2 * len(value) + 2))
        offsets[k] = new
        yield "offsets", k, [j for j in (k - 1, k) if 0 <= j < H]
        offsets[k] = old
    for _ in range(n_table):
        k = int(rng.integers(H))
        old = int(hashes[k])
        near = int(rng.integers(2))
        new = old
        while new == old:
            new = min(max(0, old + int(rng.integers(-2, 3))), 0xFFFFFFFF) if near else int(rng.integers(1 << 32))
        hashes[k] = new
        yield "hashes", k, []
        hashes[k] = old


# ---- the oracle's indices ----------------------------------------------------------------------------------------------------------------
def oracle_index(kind):
    """(value, hashes, offsets, n_structures) of the oracle's index over the serine peptidases ("serine") or 600 synthetic structures ("synth600")"""
    import oracle
    from tests import helpers
    structs = [oracle.read_pdb(p) for p in helpers.SER] if kind == "serine" else helpers.packed_to_oracle_structs(helpers.synthetic_packed(600, 7))
    ix, _, _ = oracle.build_index(structs)
    return ix.values().copy(), ix.hashes().copy(), ix.offsets().copy(), len(structs)
