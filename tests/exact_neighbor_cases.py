"""Hand-made rows for the exact neighbour tests (device and host), independent of any build: a universe of ascending hashes that includes 0
and 0xFFFFFFFF, S = 600 rows prescribed as subsets of it, the index that holds them at the first ids 0 and 16200 (so that ids cross the
2- / 3-byte varint edge at 16,384; the rows transposed to id lists and encoded with the LEB128 helpers of the rebase cases), and a second
small index for --against.  Expected values come from Python sets (indexio.row_neighbors_from_rows).  Structure k of the index (id first_id
+ k) has the row ROWS[k]; NAMES maps a case's name to its k.  The module asserts at import that every edge it is made for is present.

The layout, by position k:
  0, 300, 598, 599   empty rows
  1 .. 549           the crowd (but 300): every row holds the two CROWD hashes, the index's first and last hash, whose lists of about 550 bytes
                     cross the walk's 256- and 512-byte steps; 1 .. 255 and 455 hold STRADDLE[0], 1 .. 254 and 455 hold STRADDLE[16200]: the
                     list in which, at that first id, a two-byte delta lies on bytes 255 and 256
    1 .. 20, 21 .. 40  two graded families: a core of 200 hashes, member m drops the first m of them and adds m private ones
    41 .. 47           twins: (41, 42), (43, 44, 45), (46, 47) have equal rows
    50 .. 55           rows of exactly 63, 64, 65, 128, 129 and 1000 hashes, the chunk edges of the count kernel
    the others         random subsets of a pool of 1,500 hashes
  550 .. 589         islands (no crowd hash): a graph whose every edge is one hash held by its two ends and by nobody else, so a node's
                     candidates inside the index are its graph neighbours, each with inter = 1.  550 has no edge; the hubs 551 .. 556 have 7, 8, 9,
                     31, 32 and 33 edges to the leaves 557 .. 589 (a hub of m edges to the first m leaves), which leaves the last two leaves
                     with 2 and 1: fewer than, exactly and more than k candidates for k = 1, 8 and 32.  Leaves with equally many edges tie fully
                     and are ordered by id; the hubs of 9 and 33 edges have such a tie exactly at the k-th place for k = 8 and 32, the triple
                     of twins for k = 1
  590 .. 592         tie_q = 4 hashes; tie_x shares 2 of them and has a union of 4, tie_y shares 3 and has a union of 6: 2 * 6 == 3 * 4
  593                one hash that no other row holds: a row of length 1, a list of 1 id
  594, 595           twins of one hash
  596, 597           two rows around one hash, the second with one more"""
import numpy as np

from tests.rebase_cases import decode, encode      # noqa: F401

FIRST_IDS = (0, 16200)
S = 600
TOP = 0xFFFFFFFF
QUERY_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 1000)
HUBS = (7, 8, 9, 31, 32, 33)                          # edges of the hubs 551 .. 556
KS = (1, 8, 32)
FLOORS = (0, 1, 5000, 10000)


def _universe():
    rng = np.random.Generator(np.random.PCG64(20250611))
    mid = set()
    while len(mid) < 5996:
        mid.update(int(x) for x in rng.integers(256, TOP - 256, size=5996 - len(mid), dtype=np.uint64))
    return [0, 1] + sorted(mid) + [TOP - 1, TOP]


U = _universe()
CROWD = (U[2], U[-3])                                 # the first and the last hash of the index
STRADDLE = {0: U[3], 16200: U[4]}
CORES = (U[100:300], U[300:500])
POOL = U[500:2000]
NOLIST = U[2000:2100]                                 # hashes in no list of the index
_PRIVATE = iter(U[2100:-3])


def _make_rows():
    rng = np.random.Generator(np.random.PCG64(11))
    rows, names = [None] * S, {}

    def put(k, name, row):
        assert rows[k] is None and name not in names and len(set(row)) == len(row)
        names[name] = k
        rows[k] = sorted(row)

    def private(n):
        return [next(_PRIVATE) for _ in range(n)]

    def crowd(k, extra):
        return set(CROWD) | ({STRADDLE[0]} if 1 <= k <= 255 or k == 455 else set()) | ({STRADDLE[16200]} if 1 <= k <= 254 or k == 455 else set()) | set(extra)
    for k in (0, 300, 598, 599):
        put(k, f"empty{k}", [])
    for f, core in enumerate(CORES):                  # graded families
        for m in range(20):
            k = 1 + 20 * f + m
            put(k, f"fam{f}_{m}", crowd(k, core[m:] + private(m)))
    for group in ((41, 42), (43, 44, 45), (46, 47)):  # twins: equal rows (the straddle hashes are held by all of 1 .. 254)
        extra = [POOL[int(i)] for i in rng.choice(len(POOL), size=40, replace=False)]
        for k in group:
            put(k, f"twin{k}", crowd(k, extra))
    for k, L in zip(range(50, 56), QUERY_LENGTHS[2:]):
        base = crowd(k, [])
        put(k, f"len{L}", list(base) + [POOL[int(i)] for i in rng.choice(len(POOL), size=L - len(base), replace=False)])
    for k in range(1, 550):
        if rows[k] is None:
            n = int(rng.integers(5, 300))
            put(k, f"rand{k}", crowd(k, [POOL[int(i)] for i in rng.choice(len(POOL), size=n, replace=False)]))
    node = {550: private(1)}                          # the islands' graph: one hash per edge
    for hub, m in zip(range(551, 557), HUBS):
        for leaf in range(557, 557 + m):
            edge = private(1)
            node.setdefault(hub, []).extend(edge)
            node.setdefault(leaf, []).extend(edge)
    put(550, "lone", node[550])
    for hub, m in zip(range(551, 557), HUBS):
        put(hub, f"hub{m}", node[hub])
    for leaf in range(557, 590):
        put(leaf, f"leaf{leaf - 556}", node[leaf])
    t = private(6)
    put(590, "tie_q", t[:4])
    put(591, "tie_x", t[:2])
    put(592, "tie_y", t[:3] + t[4:6])
    put(593, "len1", private(1))
    twin = private(1)
    put(594, "twin594", twin)
    put(595, "twin595", twin)
    pair = private(2)
    put(596, "pair_a", pair[:1])
    put(597, "pair_b", pair)
    assert all(r is not None for r in rows)
    return rows, names


ROWS, NAMES = _make_rows()
SETS = [frozenset(r) for r in ROWS]
LENGTHS = np.array([len(r) for r in ROWS], np.uint32)

# the queries the tests ask: every planted case and every eleventh structure of the rest of the crowd
QUERIES = np.array(sorted(set(range(0, 60)) | {183, 184, 185, 254, 255, 256, 300, 455, 549} | set(range(550, 600)) | set(range(60, 550, 11))), np.int64)


def _make_against():
    """the second, small index: rows that reach beyond the first one's hashes on both sides"""
    rng = np.random.Generator(np.random.PCG64(12))
    rows = [[0, TOP] + list(CROWD),                   # 0 and 0xFFFFFFFF themselves, and the first index's first and last hash
            [0], [TOP], [1, TOP - 1],                 # below its first hash, above its last: no list is found
            [],
            list(ROWS[NAMES["len64"]]),               # a row of the first index as it is: the same set
            list(ROWS[NAMES["fam0_3"]]) + NOLIST[:5], # one with hashes in no list
            NOLIST[5:40],                             # only such hashes
            list(ROWS[NAMES["tie_q"]]), list(ROWS[NAMES["hub9"]]), list(ROWS[NAMES["len1000"]])[::2] + [0, 1]]
    while len(rows) < 40:
        n = int(rng.integers(3, 200))
        rows.append([POOL[int(i)] for i in rng.choice(len(POOL), size=n, replace=False)] + ([TOP] if len(rows) % 3 == 0 else []))
    return [sorted(set(r)) for r in rows]


AGAINST_ROWS = _make_against()
AGAINST_FIRST = 7


def _lists_of(rows, first_id):
    lists = {}
    for s, row in enumerate(rows):
        for h in row:
            lists.setdefault(h, []).append(first_id + s)
    return lists


def _index_of(rows, first_id):
    return index_of_lists(_lists_of(rows, first_id))


def index_of_lists(lists):
    """{hash: ascending ids} -> (value, hashes, offsets)"""
    hashes = sorted(lists)
    blobs = [encode(lists[h]) for h in hashes]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), np.array(hashes, np.uint32), off


def index(first_id: int):
    """the index that holds ROWS at the ids first_id .. first_id + S - 1 -> (value, hashes, offsets)"""
    return _index_of(ROWS, first_id)


def against_index():
    """the second index: AGAINST_ROWS at the ids AGAINST_FIRST .. -> (value, hashes, offsets)"""
    return _index_of(AGAINST_ROWS, AGAINST_FIRST)


def sub_index(lo: int, hi: int, first_id: int):
    """an index of its own over ROWS[lo: hi] at the ids first_id .. -> (value, hashes, offsets)"""
    return _index_of(ROWS[lo:hi], first_id)


def csr(rows):
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return np.array([h for r in rows for h in r], np.uint32), off


def rows_csr(ks=None):
    """the rows ks (default: all, in order) as CSR"""
    return csr([ROWS[int(k)] for k in (range(S) if ks is None else ks)])


def varint_spans(blob: bytes):
    """(first byte, byte length) of every varint of a list"""
    out, start = [], 0
    for p, b in enumerate(blob):
        if not b & 0x80:
            out.append((start, p + 1 - start))
            start = p + 1
    return out


def ranked(q: int, exclude_self: bool = True):
    """the candidates of structure q inside the index at floor 0 as (inter, union, k), nearest first, by Python sets and exact fractions"""
    from fractions import Fraction
    c = []
    for s in range(S):
        i = len(SETS[q] & SETS[s])
        if i and not (exclude_self and s == q):
            c.append((-Fraction(i, len(SETS[q] | SETS[s])), -i, s, len(SETS[q] | SETS[s])))
    return [(-ni, u, s) for _, ni, s, u in sorted(c)]


def _check():
    assert U == sorted(set(U)) and U[0] == 0 and U[-1] == TOP and len(ROWS) == S and all(r == sorted(set(r)) and set(r) <= set(U) for r in ROWS)
    used = set().union(*SETS)
    assert not used & ({0, 1, TOP - 1, TOP} | set(NOLIST)) and min(used) == CROWD[0] and max(used) == CROWD[1]      # what --against reaches beyond
    assert set(QUERY_LENGTHS) <= {int(LENGTHS[k]) for k in QUERIES}
    for f in FIRST_IDS:
        lists = _lists_of(ROWS, f)
        for h in CROWD:                               # held by every structure of the crowd: the list crosses the 256- and the 512-byte step
            assert len(lists[h]) == 548 and 512 < len(encode(lists[h])) < 768
        blob = encode(lists[STRADDLE[f]])
        assert (255, 2) in varint_spans(blob) and decode(blob) == lists[STRADDLE[f]], f      # a two-byte delta on bytes 255 and 256
        assert sum(len(v) == 1 for v in lists.values()) > 100                                # lists of 1 id
    heads = {len(encode([16200 + k])) for k in range(S)}
    assert heads == {2, 3}                                                                   # ids on both sides of 16,384
    for f, core in enumerate(CORES):
        for m in range(20):
            r = SETS[NAMES[f"fam{f}_{m}"]]
            assert len(r & set(core)) == 200 - m and len(r) == 204
    for a, b in ((41, 42), (43, 44), (44, 45), (46, 47), (594, 595)):
        assert SETS[a] == SETS[b] and SETS[a]
    # the product tie: 2 / 4 against 3 / 6, the larger inter first
    assert ranked(NAMES["tie_q"]) == [(3, 6, NAMES["tie_y"]), (2, 4, NAMES["tie_x"])]
    # candidate counts around every k, full ties ordered by id, and a tie exactly at the k-th place
    counts = {name: len(ranked(NAMES[name])) for name in ["lone", "leaf33", "leaf32"] + [f"hub{m}" for m in HUBS]}
    assert counts == {"lone": 0, "leaf33": 1, "leaf32": 2, "hub7": 7, "hub8": 8, "hub9": 9, "hub31": 31, "hub32": 32, "hub33": 33}
    assert set(counts.values()) >= {k + d for k in KS for d in (-1, 0, 1)}
    for m in HUBS:
        r = ranked(NAMES[f"hub{m}"])
        assert all(i == 1 for i, _, _ in r) and [s for _, _, s in r] == sorted((s for _, _, s in r), key=lambda s: (len(SETS[s]), s))
    for k, q in zip(KS, (43, NAMES["hub9"], NAMES["hub33"])):
        r = ranked(q)
        assert len(r) > k and r[k - 1][:2] == r[k][:2] and r[k - 1][2] < r[k][2]
    assert ranked(43)[0][:2] == (len(SETS[43]), len(SETS[43]))                               # the twins: inter == union
    assert ranked(NAMES["len1"]) == [] and ranked(0) == []
    assert not AGAINST_ROWS[4] and set(AGAINST_ROWS[5]) == SETS[NAMES["len64"]] and not set(AGAINST_ROWS[7]) & used and len(AGAINST_ROWS) == 40


_check()


# ---- what the CPU and the GPU test file share around the cases
_STATED = {}
_INTER = []


def statement(first_id, k, T, queries=None, exclude_self=True):
    """the plain statement (indexio.row_neighbors_from_rows) for the queries (positions of ROWS; default QUERIES) inside the hand-made index.
    For the default queries it is stated once per (first_id, k, T, exclude_self), shared by the tests and left unchanged"""
    from folddisco_amd import indexio
    key = (first_id, k, T, exclude_self) if queries is None else None
    if key is None or key not in _STATED:
        q = QUERIES if queries is None else np.asarray(queries)
        got = indexio.row_neighbors_from_rows(rows_csr(q), rows_csr(), first_id, k, T, (first_id + q).astype(np.uint32) if exclude_self else None)
        got.setflags(write=False)
        if key is None:
            return got
        _STATED[key] = got
    return _STATED[key]


def intersections():
    """|R_q ∩ R_s| for q in QUERIES and every s, by Python sets, u32 (len(QUERIES), S); made once"""
    if not _INTER:
        m = np.array([[len(SETS[int(q)] & SETS[s]) for s in range(S)] for q in QUERIES], np.uint32)
        m.setflags(write=False)
        _INTER.append(m)
    return _INTER[0]


def status(argv):
    """the exit status of `python -m folddisco_amd ARGV`, run in this process"""
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


def write_index(prefix, rows=None, tids=None):
    """an index over the rows (default: the hand-made ones) as files, ids from 0 -> its tids"""
    from folddisco_amd import indexio
    v, h, o = index(0) if rows is None else _index_of(rows, 0)
    n = S if rows is None else len(rows)
    indexio.write_index_files(prefix, v, h, o)
    tids = tids or [f"t{k}" for k in range(n)]
    indexio.save_lookup_py(prefix + ".lookup", tids, 50 + np.arange(n, dtype=np.uint64), np.full(n, 80.5, np.float32))
    indexio.save_type(prefix + ".type", n)
    return tids


def damaged_index(first_id):
    """the hand-made index with one list, of a hash that structure 43 holds, whose last id is first_id + S: outside the index"""
    lists = _lists_of(ROWS, first_id)
    h = ROWS[43][5]
    lists[h] = lists[h][:-1] + [first_id + S]
    return index_of_lists(lists)


def exact_tsv(nb, ids, tids_q, tids_d, len_q, len_d):
    """the TSV `neighbors --exact` writes for the records nb of the queries ids"""
    lines = []
    for q, row in enumerate(nb):
        for rank, r in enumerate(row):
            if int(r["id"]) == 0xFFFFFFFF:
                break
            i, u, s = int(r["inter"]), int(r["union"]), int(r["id"])
            lines.append("\t".join([str(int(ids[q])), tids_q[int(ids[q])], str(int(len_q[int(ids[q])])), str(rank + 1), str(s), tids_d[s], str(int(len_d[s])),
                                    str(i), str(u), f"{i / max(u, 1):.4f}", "identical" if int(r["flags"]) & 1 else "similar"]) + "\n")
    return "".join(lines)
