"""Hand-made rows for the exact row overlap tests (device and host), independent of any build: a universe of 9,000 ascending hashes that
includes 0, 1, 0xFFFFFFFE and 0xFFFFFFFF, 64 rows prescribed as subsets of it, the index that holds them (the rows transposed to id lists and
encoded with the LEB128 helpers of the rebase cases; the hashes are the universe's, not pack's 3 k + 1), and the expected overlaps by Python
sets.  Structure k of the index (id first_id + k) has the row ROWS[k]; NAMES maps a case's name to its k."""
import numpy as np

from tests.rebase_cases import decode, encode      # noqa: F401

FIRST_IDS = (0, 5)
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 1000, 4200)
N = 64
TOP = 0xFFFFFFFF


def _universe():
    rng = np.random.Generator(np.random.PCG64(20241020))
    mid = set()
    while len(mid) < 8996:
        mid.update(int(x) for x in rng.integers(2, TOP - 1, size=8996 - len(mid), dtype=np.uint64))
    return [0, 1] + sorted(mid) + [TOP - 1, TOP]


U = _universe()


def _make_rows():
    rng = np.random.Generator(np.random.PCG64(7))
    rows, names = [], {}

    def add(name, row):
        assert row == sorted(set(row)) and name not in names
        names[name] = len(rows)
        rows.append(row)
    for L in LENGTHS:                                 # a contiguous run of the universe per length, and a second structure with the same row
        add(f"len{L}", U[100:100 + L])
        add(f"copy{L}", U[100:100 + L])
    add("evens", U[0::2])                             # disjoint and interleaved; 0 and 0xFFFFFFFE here, 1 and 0xFFFFFFFF there
    add("odds", U[1::2])
    add("low", U[0:1000])                             # disjoint by range
    add("high", U[5000:6000])
    add("third", U[100:4300:3])                       # every third element of len4200
    add("first_a", [U[50]] + U[1000:1200:2])          # the only common element first in both
    add("first_b", [U[50]] + U[1001:1201:2])
    add("last_a", U[1000:1200:2] + [U[8000]])         # last in both
    add("last_b", U[1001:1201:2] + [U[8000]])
    add("cross_a", [U[3000]] + U[3001:3201:2])        # first in one, last in the other
    add("cross_b", U[2000:2200] + [U[3000]])
    # four common elements, at the positions 63, 64, 127 and 128 of both edge_p and edge_q: a match on each side of two tile edges
    p = U[4000:4400:2]
    add("edge_p", p)
    q = U[3000:3063] + [p[63], p[64]] + U[4129:4253:2] + [p[127], p[128]] + U[4257:4300:2]
    add("edge_q", q)
    add("edge_q1", q[1:])                             # the same elements one position earlier: 62, 63, 126, 127
    add("ends_a", [0] + U[6000:6100] + [TOP])         # 0 and 0xFFFFFFFF in both rows, in one only, in neither
    add("ends_b", [0] + U[6050:6150] + [TOP])
    add("mid_a", U[6000:6100])
    add("mid_b", U[6050:6150])
    add("zero", [0])
    add("top", [TOP])
    add("one_in", [U[100 + 77]])                      # 1 against 4200: an element of len4200
    while len(rows) < N:                              # random rows of random sizes
        k = int(rng.integers(5, 300))
        add(f"rand{len(rows)}", sorted(U[i] for i in rng.choice(len(U), size=k, replace=False).tolist()))
    return rows, names


ROWS, NAMES = _make_rows()
SETS = [set(r) for r in ROWS]

# the cases the issue names, (row a, row b, expected overlap); every one is also checked against the sets
NAMED = [("edge_p", "edge_q", 4), ("edge_q", "edge_p", 4), ("edge_p", "edge_q1", 4), ("edge_q1", "edge_p", 4),
         ("evens", "odds", 0), ("odds", "evens", 0), ("low", "high", 0), ("high", "low", 0), ("len4200", "third", 1400), ("third", "len4200", 1400),
         ("first_a", "first_b", 1), ("last_a", "last_b", 1), ("cross_a", "cross_b", 1), ("cross_b", "cross_a", 1),
         ("len0", "copy0", 0), ("len0", "len4200", 0), ("len4200", "len0", 0), ("len1", "len0", 0),
         ("ends_a", "ends_b", 52), ("ends_a", "mid_a", 100), ("mid_a", "ends_b", 50), ("mid_a", "mid_b", 50), ("zero", "ends_a", 1), ("top", "ends_a", 1),
         ("zero", "top", 0), ("zero", "len0", 0), ("zero", "mid_a", 0), ("top", "mid_a", 0), ("zero", "evens", 1), ("top", "odds", 1), ("top", "evens", 0),
         ("one_in", "len4200", 1), ("len4200", "one_in", 1), ("one_in", "third", 0)] + \
        [(f"len{L}", f"copy{L}", L) for L in LENGTHS] + [(f"len{L}", f"len{L}", L) for L in LENGTHS]


def named_pairs():
    """-> (ka, kb, expected) of NAMED as arrays of row indices"""
    return (np.array([NAMES[a] for a, _, _ in NAMED], np.uint32), np.array([NAMES[b] for _, b, _ in NAMED], np.uint32),
            np.array([w for _, _, w in NAMED], np.uint32))


def all_pairs():
    """every ordered pair of rows, (k, k) included, row-major -> (ka, kb)"""
    k = np.arange(N, dtype=np.uint32)
    return np.repeat(k, N), np.tile(k, N)


def expected(ka, kb):
    """the pure-Python expectation: len(set & set) per pair"""
    return np.array([len(SETS[int(a)] & SETS[int(b)]) for a, b in zip(ka, kb)], np.uint32)


def work(ka, kb):
    return np.array([len(ROWS[int(a)]) + len(ROWS[int(b)]) for a, b in zip(ka, kb)], np.int64)


def index(first_id: int):
    """the index that holds ROWS at the ids first_id .. first_id + N - 1 -> (value, hashes, offsets)"""
    lists = {}
    for s, row in enumerate(ROWS):
        for h in row:
            lists.setdefault(h, []).append(first_id + s)
    hashes = sorted(lists)
    blobs = [encode(lists[h]) for h in hashes]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), np.array(hashes, np.uint32), off


def rows_csr(ks=None):
    """the rows ks (default: all, in order) as CSR"""
    ks = range(N) if ks is None else [int(k) for k in ks]
    off = np.zeros(len(ks) + 1, np.uint64)
    off[1:] = np.cumsum([len(ROWS[k]) for k in ks])
    return np.array([h for k in ks for h in ROWS[k]], np.uint32), off
