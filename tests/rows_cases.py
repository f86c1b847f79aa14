"""Hand-made posting lists for the index rows tests (device and host), independent of any build, and the expected rows by a pure-Python
transposition of the decoded lists.  The LEB128 helpers are those of the rebase cases.

Ids are relative to the index's first_id here; lists(first_id) adds it.  The index has N = 2^24 + 1 structures; everything of interest sits around
B, so that windows of every radix-pass count (widths 1, 2, 256, 257, 65536, 65537, 2^24 + 1: zero to four passes) cut through the same lists."""
import numpy as np

from tests.rebase_cases import decode, encode, pack, varint      # noqa: F401  (pack and varint: for the tests)

N = (1 << 24) + 1
B = 100000
FIRST_IDS = (0, 5)
LENGTHS = [1, 2, 255, 256, 257, 511, 513, 4200]      # byte lengths that cross the walk's 256-byte step
DENSE = list(range(B + 10, B + 310))                 # the same 300 consecutive ids in eight lists
N_DENSE = 8
# structures that occur in no list: B first in [B, B + 256), B + 5 in its middle, B + 310 last in [B + 54, B + 311); N - 2 next to the last id
HOLES = (B, B + 5, B + 310, N - 2)
EMPTY = (N - 1000, N - 500)                          # a window without any posting

# windows [lo, hi) relative to first_id
WINDOWS = [
    (B + 57, B + 58),                    # width 1 inside the dense lists: no sort pass
    (B + 5, B + 6),                      # width 1, an empty row
    (B + 9, B + 11),                     # width 2: cuts the dense lists' head
    (B, B + 256),                        # width 256: one pass
    (B + 54, B + 311),                   # width 257: two passes; ends on a hole
    (B - 30000, B + 35536),              # width 65536: two passes
    (B + 300, B + 300 + 65537),          # width 65537: three passes; cuts the dense lists' tail
    (B + 20, B + 20),                    # width 0
    EMPTY,
    (0, 2), (N - 2, N),                  # the index's two ends
    (0, N),                              # the whole index: width 2^24 + 1, four passes
]
# the windows around B, for which lists wholly below, wholly above and across either edge exist (test_hand_made_index_has_the_edges)
EDGE_WINDOWS = [w for w in WINDOWS if B - 30000 <= w[0] < w[1] <= B + 300 + 65537]


def _grow(ids, until_bytes, rng, two_byte_share=0.3):
    """append ascending ids with one- and two-byte deltas until the encoding has until_bytes bytes; no id of HOLES"""
    n = len(encode(ids))
    while n < until_bytes:
        two = until_bytes - n >= 2 and rng.random() < two_byte_share
        d = int(rng.integers(128, 290)) if two else int(rng.integers(1, 120))
        while ids[-1] + d in HOLES:
            d += 1
        ids.append(ids[-1] + d)
        n += 2 if two else 1
    assert n == until_bytes
    return ids


def _rel_lists():
    rng = np.random.Generator(np.random.PCG64(20240607))
    out = []
    # 1. the byte lengths; heads (two- and three-byte varints) below and inside the windows around B
    for k, n in enumerate(LENGTHS):
        head = 40 + k if n == 1 else (200 + k if n == 2 else B - 30000 + 3500 * k)
        out.append(_grow([head], n, rng))
    # 2. a two-byte varint across the first step edge (bytes 255, 256) and a three-byte one across the second (bytes 510 .. 512)
    ids = _grow([B - 300], 255, rng, two_byte_share=0.0)
    ids.append(ids[-1] + 200)
    ids = _grow(ids, 510, rng, two_byte_share=0.0)
    ids.append(ids[-1] + 20000)
    out.append(_grow(ids, 530, rng))
    # 3. the dense lists
    out += [list(DENSE) for _ in range(N_DENSE)]
    # 4. wholly below, wholly above, across either edge of the windows around B; the index's first and last id
    out.append([3, 50, 90])
    out.append([0, N - 1])                                   # a four-byte delta
    out.append(_grow([B + 300 + 65537 + 10], 40, rng))
    out.append(_grow([B - 30000 - 50], 200, rng))
    out.append([B - 1, B + 1, B + 255, B + 256, B + 311, B + 35535, B + 35536, B + 300 + 65536, B + 300 + 65537])
    out.append([N - 3, N - 1])
    # 5. a final one-byte list that ends on the last value byte (first_id + 7 < 128)
    out.append([7])
    return out


_REL = _rel_lists()


def lists(first_id: int):
    """the id lists in hash order (list k gets hash 3 k + 1 from pack), absolute ids"""
    return [[first_id + x for x in l] for l in _REL]


def expected_rows(id_lists, hashes, lo: int, hi: int):
    """the transposition in plain Python: every list decoded from its own bytes, its ids inside [lo, hi) appended to their rows in list (= hash)
    order -> (hashes u32, row_off u64[hi - lo + 1])"""
    rows = {}
    for l, h in zip(id_lists, hashes):
        for x in decode(encode(l)):
            if lo <= x < hi:
                rows.setdefault(x - lo, []).append(int(h))
    cnt = np.zeros(hi - lo + 1, np.uint64)
    flat = []
    for s in sorted(rows):
        cnt[s + 1] = len(rows[s])
        flat += rows[s]
    return np.array(flat, np.uint32), np.cumsum(cnt, dtype=np.uint64)
