"""Hand-made posting lists for the index merge (fdgpu_index_merge, fdgpu_merge_subindices) and the hash-range slicing behind the single index
(fdgpu_index_range_bounds / _slice / _save_part), independent of any build.  A part is (first_id, n_structures, {hash: ascending absolute ids});
a merge is a tuple of parts over consecutive id ranges.  The model is list-level Python: per hash, in ascending hash order, the ids decoded again
from each part's own bytes are concatenated, delta-encoded and LEB128-encoded (the codec of tests/rebase_cases.py).  The families put the cases
where the merge's kernels decide something:

  junction    the first varint of a continuation, re-based from an absolute id of a bytes to a delta of d bytes: all 15 pairs d <= a, a delta on
              both sides of every 7-bit boundary, pieces of every ragged-tail length of fd_list_copy behind the new head (and the head alone),
              and ids next to 2^31 and at the top of the id space (five-byte deltas, which the step cases of tests/postings_step_cases.py
              leave out, are reached here: nothing in a merge is allocated per structure)
  last_step   lists of a LOADED part whose last ids k_mg_last_ids has to derive: one wide varint across or beside the edge of its 64-byte step,
              as the last varint or before a dozen more, and lists that end on, before and behind the edge; every list goes on in the next part,
              because a wrong last id shows only as a wrong first delta there
  presence    which parts hold a hash: every non-empty subset of three parts, 64 parts (the limit), empty parts in every place, one part alone
  hash_space  the bitmap: hashes at word edges, a word whose bits alternate between the parts, the largest hash on both sides of the switch
              between the 2^30-bit and the 2^32-bit bitmap, hash 0xffffffff

and probe_part builds, for the result of any other operation, the part that follows it with one id per list: merged with it, the result shows the
last ids it carries.  Everything is deterministic (PCG64 with fixed seeds), computed once per process and never written to disk; callers leave the
arrays as they are.  Every generator asserts the coverage it is there for, so that an edit cannot lose a case silently."""
import functools

import numpy as np

from tests.rebase_cases import LENGTHS, decode, encode, varint

MAX_PARTS = 64                                          # MG_MAX_PARTS of k_merge.hip
NARROW_WORDS, WIDE_WORDS = 1 << 25, 1 << 27             # bitmap words: 2^30 bits, 2^32 bits from a largest hash of 2^30 on
BOUNDARIES = (1 << 7, 1 << 14, 1 << 21, 1 << 28)
ID_TOP = (1 << 32) - 1                                  # first_id + n_structures may reach this: the library keeps id 0xffffffff free


# ---- parts, arrays and the model
def pack_part(part):
    """(first_id, n_structures, {hash: ids}) -> (value, hashes, offsets), the lists in ascending hash order"""
    lists = part[2]
    hs = sorted(lists)
    blobs = [encode(lists[h]) for h in hs]
    off = np.zeros(len(hs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), np.array(hs, np.uint32), off


def lists_of(arrays):
    """(value, hashes, offsets) -> {hash: ids}, decoded from the bytes"""
    v, h, o = arrays
    raw = np.asarray(v, np.uint8).tobytes()
    return {int(h[k]): decode(raw[int(o[k]):int(o[k + 1])]) for k in range(len(h))}


def as_part(first_id: int, n_structures: int, arrays):
    return (first_id, n_structures, lists_of(arrays))


def merged_part(parts):
    per = [lists_of(pack_part(p)) for p in parts]          # decoded from each part's own bytes: the expectation does not rest on the generators
    out = {h: [x for d in per if h in d for x in d[h]] for h in sorted(set().union(*per))}
    return (parts[0][0], sum(p[1] for p in parts), out)


def merged(parts):
    """the model: (value, hashes, offsets) of the merge of the parts"""
    return pack_part(merged_part(parts))


def n_postings(arrays) -> int:
    return sum(len(l) for l in lists_of(arrays).values())


def file_bytes(value, hashes, offsets):
    """the two files of an index: PREFIX = the value bytes, PREFIX.offset = u64 H | u32 hashes[H] | u64 offsets[H + 1]"""
    return (np.ascontiguousarray(value, np.uint8).tobytes(),
            np.uint64(len(hashes)).tobytes() + np.ascontiguousarray(hashes, np.uint32).tobytes() + np.ascontiguousarray(offsets, np.uint64).tobytes())


def bitmap_words(parts) -> int:
    return WIDE_WORDS if max((h for p in parts for h in p[2]), default=0) >= 1 << 30 else NARROW_WORDS


def probe_part(first_id: int, n_structures: int, arrays):
    """the part behind an index: one structure, which every list of the index holds"""
    nxt = first_id + n_structures
    return (nxt, 1, {int(h): [nxt] for h in arrays[1]})


def check_parts(parts):
    """consecutive ranges, every list non-empty, strictly ascending and inside its part's range"""
    for k, (f, n, lists) in enumerate(parts):
        assert k == 0 or f == parts[k - 1][0] + parts[k - 1][1]
        assert f + n <= 1 << 32
        for ids in lists.values():
            assert ids and f <= ids[0] and ids[-1] < f + n and all(a < b for a, b in zip(ids, ids[1:]))


def _tail(head: int, n_bytes: int, seed: int):
    """ascending ids from head whose encoding takes exactly n_bytes: one- and two-byte deltas behind the head"""
    room = n_bytes - len(varint(head))
    assert room >= 0
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = [head]
    while room:
        d = int(rng.integers(128, 300)) if room >= 2 and rng.random() < 0.3 else int(rng.integers(1, 128))
        ids.append(ids[-1] + d)
        room -= len(varint(d))
    assert len(encode(ids)) == n_bytes
    return ids


def _sample(lo: int, hi: int, n: int, seed: int):
    rng = np.random.Generator(np.random.PCG64(seed))
    return sorted(int(x) for x in lo + rng.choice(hi - lo, size=min(n, hi - lo), replace=False))


# ---- junction
JUNCTION_SUMS = (1, 2) + tuple(b + e for b in BOUNDARIES for e in (-1, 0))      # last id of part 0 .. first id of part 1
N_CONTINUATION = 1 << 29                                                        # structures of part 1: heads up to 2^28 - 1 above its first id


def junction_first_id(a: int) -> int:
    """first_id of part 1, just above 0, 2^7, 2^14, 2^21, 2^28: its lists' heads take a bytes"""
    return 40 + (0 if a == 1 else 1 << (7 * (a - 1)))


def _junction_merge(a: int):
    F = junction_first_id(a)
    p0, p1, k = {}, {}, 0
    for s in JUNCTION_SUMS:
        if len(varint(s)) > a:
            continue
        x, y = (s - min(s - 1, 3), min(s - 1, 3)) if s <= F else (F, s - F)      # part 0 ends at F - x, part 1 starts at F + y
        assert 1 <= x <= F and x + y == s and len(varint(F + y)) == a
        for n in sorted(set(LENGTHS) | {a}):                                     # n = a: the piece is its head alone
            if n < a:
                continue
            last0 = F - x
            p0[7 * k + 5] = [v for v in (last0 - 3 * j * j for j in reversed(range(1 + k % 4))) if v >= 0]
            p1[7 * k + 5] = _tail(F + y, n, 100000 * a + 100 * k + 1)
            k += 1
    assert max(l[-1] for l in p1.values()) < F + N_CONTINUATION
    return ((0, F, p0), (F, N_CONTINUATION, p1))


def junction_top(top: int):
    """ids next to 2^31 and below top = first_id + n_structures of the last part: a list that ends at top - 1, junction deltas of 2^31 and more"""
    F = (1 << 31) + 100
    p0 = {3: [50], 10: [0, F - 1], 17: [1 << 31], 31: [0], 38: [7, 9], 45: [(1 << 31) - 1, 1 << 31]}
    p1 = {3: [F + 10, top - 1], 10: [F], 24: [top - 1], 31: [top - 1], 38: [F + 5, F + 6], 45: [F + (1 << 21), top - 2]}
    parts = ((0, F, p0), (F, top - F, p1))
    m = merged_part(parts)[2]
    assert any(l[-1] == top - 1 for l in m.values()) and any(p1[h][0] - p0[h][-1] >= 1 << 31 for h in p0 if h in p1)
    return parts


def junction_pairs(merges):
    """{(bytes of the continuation's head in its part, bytes of its delta in the merge)}, {the deltas}; from the bytes"""
    pairs, deltas = set(), set()
    for parts in merges:
        per = [pack_part(p) for p in parts]
        dec = [lists_of(a) for a in per]
        for h in dec[1]:
            if h in dec[0]:
                d = dec[1][h][0] - dec[0][h][-1]
                pairs.add((len(varint(dec[1][h][0])), len(varint(d))))
                deltas.add(d)
    return pairs, deltas


@functools.lru_cache(maxsize=None)
def junction():
    out = {f"a{a}": _junction_merge(a) for a in range(1, 6)}
    pairs, deltas = junction_pairs(out.values())
    assert pairs == {(a, d) for a in range(1, 6) for d in range(1, a + 1)}, pairs
    assert {1, 2} <= deltas and all({b - 1, b} <= deltas for b in BOUNDARIES)
    for parts in out.values():                     # every length behind the head, the head alone, and destinations of every alignment mod 4
        a = len(varint(parts[1][0]))
        assert {len(encode(l)) for l in parts[1][2].values()} == {n for n in set(LENGTHS) | {a} if n >= a}
        assert {int(o) % 4 for o in merged(parts)[2]} == {0, 1, 2, 3}
    out["top"] = junction_top(ID_TOP)
    return out


# ---- last_step
WIDE_DELTA = {2: 1500, 3: 20000, 4: (1 << 21) + 5, 5: (1 << 28) + 5}
STEP = 64                                              # bytes per step of k_mg_last_ids
STEP_STARTS = (60, 61, 62, 63, 64, 124, 125, 126, 127, 128)
STEP_LENGTHS = (1, 5, 63, 64, 65, 127, 128, 129, 4200)
STEP_TAIL = 12
LS_RANGES = ((0, 1 << 30), (1 << 30, 1 << 16), ((1 << 30) + (1 << 16), 1000))      # (first_id, n_structures) of the three parts


def _build(head: int, seed: int, plan):
    """plan: ("run_to", byte) one-byte deltas up to that byte, ("wide", w) one delta of w bytes, ("run", n) n one-byte deltas
    -> (ids, [(start byte, w) of every wide delta]); the bytes are checked: every wide varint starts where the plan puts it"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids, pos, wide = [head], len(varint(head)), []
    for what, arg in plan:
        if what == "wide":
            wide.append((pos, arg))
            ids.append(ids[-1] + WIDE_DELTA[arg])
            pos += arg
        else:
            n = arg - pos if what == "run_to" else arg
            assert n >= 0
            for d in rng.integers(1, 4, n):
                ids.append(ids[-1] + int(d))
            pos += n
    blob = encode(ids)
    assert len(blob) == pos
    for p, w in wide:
        assert blob[p - 1] < 0x80 and all(b >= 0x80 for b in blob[p:p + w - 1]) and blob[p + w - 1] < 0x80
    return ids, wide


@functools.lru_cache(maxsize=None)
def last_step_lists():
    """[(name, ids, wide)] of part 0 in hash order; list k gets hash 3 k + 1"""
    out = []
    for w in sorted(WIDE_DELTA):
        for p in STEP_STARTS:
            out.append((f"last_w{w}_p{p}",) + _build(3, 1000 * w + p, [("run_to", p), ("wide", w)]))
            out.append((f"tail_w{w}_p{p}",) + _build(3, 1000 * w + p + 500, [("run_to", p), ("wide", w), ("run", STEP_TAIL)]))
    for n in STEP_LENGTHS:
        plan = [] if n in (1, 5) else [("run_to", n - 2), ("wide", 2)]
        out.append((f"exact_{n}",) + _build((1 << 28) + 7 if n == 5 else 3, 9000 + n, plan))
    lens = {name: len(encode(ids)) for name, ids, _ in out}
    for w in WIDE_DELTA:
        assert len(varint(WIDE_DELTA[w])) == w
        for p in STEP_STARTS:
            assert [e[2] for e in out if e[0] in (f"last_w{w}_p{p}", f"tail_w{w}_p{p}")] == [[(p, w)], [(p, w)]]
            assert lens[f"last_w{w}_p{p}"] == p + w and lens[f"tail_w{w}_p{p}"] == p + w + STEP_TAIL      # the last varint / a dozen behind it
        for edge in (STEP, 2 * STEP):                                                                      # every straddle of the edge
            assert {p for p in STEP_STARTS if p < edge < p + w} == set(range(edge - w + 1, edge))
    assert [lens[f"exact_{n}"] for n in STEP_LENGTHS] == list(STEP_LENGTHS) and len(varint((1 << 28) + 7)) == 5
    return out


@functools.lru_cache(maxsize=None)
def last_step():
    ls = last_step_lists()
    (f0, n0), (f1, n1), (f2, n2) = LS_RANGES
    p0 = {3 * k + 1: ids for k, (_, ids, _) in enumerate(ls)}
    p1 = {3 * k + 1: [f1 + (37 * k) % 1000] + ([f1 + 2000 + k] if k % 2 else []) for k in range(len(ls))}      # EVERY list goes on in part 1
    p2 = {3 * k + 1: [f2 + (5 * k) % n2] for k in range(len(ls)) if k % 3}                                       # every third one ends there
    assert set(p1) == set(p0) and 0 < len(p2) < len(p0)
    return {"steps": ((f0, n0, p0), (f1, n1, p1), (f2, n2, p2))}


# ---- presence
def _random_part(first_id: int, n: int, hashes, seed: int):
    return (first_id, n, {h: _sample(first_id, first_id + n, (1, 2, 40, 300)[j % 4], seed + j) for j, h in enumerate(hashes)})


def holders(parts):
    """{hash: tuple of the parts that hold it}"""
    out = {}
    for k, p in enumerate(parts):
        for h in p[2]:
            out.setdefault(h, []).append(k)
    return {h: tuple(v) for h, v in out.items()}


def _with_empties(sizes, seed: int):
    """sizes: n_structures of the parts; a negative one stands for a part with that many structures and no hash"""
    parts, f = [], 7
    for k, n in enumerate(sizes):
        parts.append((f, abs(n), {}) if n <= 0 else _random_part(f, n, range(10 + k, 400, 3 + k), seed + 1000 * k))
        f += abs(n)
    return tuple(parts)


@functools.lru_cache(maxsize=None)
def presence():
    out = {}
    ranges = ((100, 1000), (1100, 50), (1150, 5000))
    lists = [{}, {}, {}]
    for mask in range(1, 8):
        for j in range(4):
            for k in range(3):
                if mask >> k & 1:
                    f, n = ranges[k]
                    lists[k][100 * mask + 9 * j] = _sample(f, f + n, (1, 2, 40, 300)[(j + k) % 4], 10000 * mask + 10 * j + k)
    out["subsets3"] = tuple((f, n, l) for (f, n), l in zip(ranges, lists))
    hold = set(holders(out["subsets3"]).values())
    assert hold == {tuple(k for k in range(3) if m >> k & 1) for m in range(1, 8)} and any(h[0] != 0 for h in hold)

    p64 = []
    for k in range(MAX_PARTS):
        l = {11: [10 * k + k % 10] + ([10 * k + 9] if k % 10 != 9 else [])}
        if k == 63:
            l[12] = [10 * k + 4]
        if k in (0, 63):
            l[13] = [10 * k + 1, 10 * k + 2]
        if k % 2 == 0:
            l[14] = [10 * k + 7]
        else:
            l[15] = [10 * k + 3]
        p64.append((10 * k, 10, l))
    out["parts64"] = tuple(p64)
    evens, odds = tuple(range(0, 64, 2)), tuple(range(1, 64, 2))
    assert holders(p64) == {11: tuple(range(64)), 12: (63,), 13: (0, 63), 14: evens, 15: odds} and len(p64) == MAX_PARTS

    out["empties_a"] = _with_empties((0, 300, -5, 300, 0), 31)          # an empty part first, in the middle and last, without structures ...
    out["empties_b"] = _with_empties((-4, 300, 0, 300, -3), 32)         # ... and with some
    for name in ("empties_a", "empties_b"):
        e = [(k, p[1]) for k, p in enumerate(out[name]) if not p[2]]
        assert [k for k, _ in e] == [0, 2, 4]
    assert {n > 0 for name in ("empties_a", "empties_b") for k, n in [(0, out[name][0][1]), (2, out[name][2][1]), (4, out[name][4][1])]} == {True, False}
    assert [p[1] for p in out["empties_a"]] == [0, 300, 5, 300, 0] and [p[1] for p in out["empties_b"]] == [4, 300, 0, 300, 3]

    out["one_part"] = (_random_part(12345, 2000, range(3, 300, 7), 77),)
    return out


# ---- hash_space
@functools.lru_cache(maxsize=None)
def hash_space():
    f = ((0, 500), (500, 500))

    def two(held, seed):
        """held: {hash: "a" | "b" | "ab"}"""
        ps = [{}, {}]
        for j, (h, who) in enumerate(sorted(held.items())):
            for k, c in enumerate("ab"):
                if c in who:
                    ps[k][h] = _sample(f[k][0], f[k][0] + f[k][1], 1 + (j + k) % 5, seed + 10 * j + k)
        return tuple((f[k][0], f[k][1], ps[k]) for k in range(2))
    words = {0: "ab", 31: "b", 32: "a", 63: "ab"}
    words.update({h: "ab"[h & 1] for h in range(96, 128)})                                  # a full word, its bits alternating between the parts
    words.update({h: ("ab", "a", "b")[h % 3] for h in range(160, 192)})                     # and one with bits of both, of one and of the other
    out = {"words": two(words, 1)}
    top30 = (1 << 30) - 1
    out["narrow_max"] = two({5: "a", top30 - 33: "b", top30 - 1: "b", top30: "ab"}, 2)      # the largest hash the 2^30-bit bitmap holds
    out["wide_min"] = two({5: "a", top30 - 33: "b", top30 - 1: "b", top30: "ab", top30 + 1: "ab"}, 2)      # the same and hash 2^30
    out["wide_top"] = two({0: "b", 1 << 31: "a", 0xfffffffe: "a", 0xffffffff: "ab"}, 3)
    hw = holders(out["words"])
    assert all(hw[h] == ((h & 1),) for h in range(96, 128)) and {hw[h] for h in range(160, 192)} == {(0,), (1,), (0, 1)}
    assert {0, 31, 32, 63} <= set(hw)
    assert max(holders(out["narrow_max"])) == top30 and max(holders(out["wide_min"])) == 1 << 30 and 0xffffffff in holders(out["wide_top"])
    assert [bitmap_words(out[n]) for n in ("words", "narrow_max", "wide_min", "wide_top")] == [NARROW_WORDS, NARROW_WORDS, WIDE_WORDS, WIDE_WORDS]
    return out


FAMILIES = {"junction": junction, "last_step": last_step, "presence": presence, "hash_space": hash_space}


NAMES = {"junction": ("a1", "a2", "a3", "a4", "a5", "top"), "last_step": ("steps",),      # stated here, so that collecting the tests generates nothing
         "presence": ("subsets3", "parts64", "empties_a", "empties_b", "one_part"), "hash_space": ("words", "narrow_max", "wide_min", "wide_top")}
ALL_CASES = [(fam, name) for fam in NAMES for name in NAMES[fam]]


def case(family: str, name: str):
    cases = FAMILIES[family]()
    assert tuple(cases) == NAMES[family]
    return cases[name]


@functools.lru_cache(maxsize=None)
def expected(family: str, name: str):
    """the model of one merge: (value, hashes, offsets), computed once per process"""
    out = merged(case(family, name))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def packed(family: str, name: str):
    """the parts of one merge as arrays"""
    out = tuple(pack_part(p) for p in case(family, name))
    for arrays in out:
        for a in arrays:
            a.setflags(write=False)
    return out
