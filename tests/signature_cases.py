"""Hand-made rows, the index that holds them, and hand-made signature tables for the index signatures tests (device and host), independent of
any build.  The expected signatures come from a pure-Python statement of the definition (include/fdgpu.h: fd_signature), with Python integers;
the expected pairs from a numpy brute force over whole tables.  The LEB128 encoder is that of the rebase cases.

Ids are relative to the index's first_id here.  The index has N = 700 structures: 1 .. 599 are the BULK (random short rows, and the members of
five lists whose byte lengths cross the walk's 256-byte step), 600 .. 611 the SPECIAL rows below, the rest of 600 .. 699 and HOLES are empty."""
import numpy as np

from tests.rebase_cases import decode, encode      # noqa: F401

N = 700
FIRST_IDS = (0, 5)
HOLES = (0, 350, N - 1)                            # empty rows at the first id, in the middle and at the last id
LIST_BYTES = (1, 255, 256, 257, 513)               # byte lengths of five lists (one byte per id: heads below 128 - 5, deltas below 128)
WINDOWS = (1, 2, 257, N)
# sub-ranges [lo, hi) whose edges fall on an empty row
RANGES = [(0, N), (0, 1), (0, 351), (350, 351), (350, N), (351, N - 1), (N - 1, N), (1, 350), (600, 612), (612, 612)]
MASK = (1 << 64) - 1
EMPTY = 0xffffffff

ONE, R63, R64, R65, LONG, ONE_BUCKET, ALL_BUCKETS, SWAPPED, SAME_A, SAME_B, NEAR_A, NEAR_B = range(600, 612)
N_LONG = 5000


def mix(h: int) -> int:
    """m(h), the splitmix64 finaliser, with Python integers"""
    z = (h + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def bucket(h: int) -> int:
    return mix(h) >> 58


def value(h: int) -> int:
    return (mix(h) >> 26) & 0xffffffff


def signature_of(row):
    """the definition: -> (n, d0, d1, sk[64]) of a set of hashes"""
    d0 = d1 = 0
    sk = [EMPTY] * 64
    for h in row:
        m = mix(h)
        d0 = (d0 + m) & MASK
        d1 ^= m
        sk[m >> 58] = min(sk[m >> 58], (m >> 26) & 0xffffffff)
    return len(row), d0, d1, sk


def table_of(rows, dtype):
    """rows (a list of hash collections) -> the expected table"""
    out = np.zeros(len(rows), dtype)
    for s, row in enumerate(rows):
        n, d0, d1, sk = signature_of(row)
        out[s] = (n, 0, d0, d1, sk)
    return out


def _make_rows():
    rng = np.random.Generator(np.random.PCG64(20240913))
    rows = [set() for _ in range(N)]
    used = set()

    def fresh(k):
        out = []
        while len(out) < k:
            h = int(rng.integers(0, 1 << 32))
            if h not in used:
                used.add(h)
                out.append(h)
        return out
    # the searched hashes first (small values, found by brute force over m(h)), so that nothing random collides with them
    by_bucket = {}
    h = 0
    while len(by_bucket) < 64 or min(len(v) for v in by_bucket.values()) < 12:
        by_bucket.setdefault(bucket(h), []).append(h)
        h += 1
    used.update(range(h))
    rows[ONE_BUCKET] = set(by_bucket[7][:10])                                  # every hash in bucket 7
    rows[ALL_BUCKETS] = {by_bucket[b][0] for b in range(64)} | {by_bucket[b][1] for b in range(0, 64, 3)}
    swapped = next((a, c) for b in range(64) for a in by_bucket[b] for c in by_bucket[b] if a < c and value(c) < value(a))
    rows[SWAPPED] = set(swapped)                                               # one bucket, the smaller v belongs to the larger h
    rows[ONE] = set(fresh(1))
    rows[R63], rows[R64], rows[R65] = set(fresh(63)), set(fresh(64)), set(fresh(65))
    rows[LONG] = set(fresh(N_LONG))
    rows[SAME_A] = set(fresh(200))
    rows[SAME_B] = set(rows[SAME_A])
    rows[NEAR_A] = set(fresh(150))
    rows[NEAR_B] = rows[NEAR_A] | set(fresh(1))                                # differs in exactly one hash
    bulk = [s for s in range(1, 600) if s not in HOLES]
    for nbytes in LIST_BYTES:                                                  # one byte per id
        (h1,) = fresh(1)
        for s in bulk[:nbytes]:
            rows[s].add(h1)
    for h1 in fresh(300):                                                      # random short lists over the bulk
        for s in rng.choice(bulk, size=int(rng.integers(1, 40)), replace=False).tolist():
            rows[s].add(h1)
    return [sorted(r) for r in rows], swapped


ROWS, SWAPPED_PAIR = _make_rows()


def index(first_id: int):
    """the index that holds ROWS at the ids first_id .. first_id + N - 1 -> (value, hashes, offsets, id lists in hash order)"""
    lists = {}
    for s, row in enumerate(ROWS):
        for h in row:
            lists.setdefault(h, []).append(first_id + s)
    hashes = sorted(lists)
    blobs = [encode(lists[h]) for h in hashes]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), np.array(hashes, np.uint32), off, [lists[h] for h in hashes]


def rows_csr(lo=0, hi=N):
    off = np.zeros(hi - lo + 1, np.uint64)
    off[1:] = np.cumsum([len(ROWS[s]) for s in range(lo, hi)])
    return np.array([h for s in range(lo, hi) for h in ROWS[s]], np.uint32), off


# ---- hand-made signature tables for the compare
PAIR_SIZES = (1, 63, 64, 65, 129)
THRESHOLDS = (1, 48, 64)


def pair_table(n: int, seed: int, dtype):
    """n records.  The first ten are planted (thr64 = 48 = 0.75):
    0 base, all 64 buckets filled | 1 agrees with 0 in 48 buckets: exactly on the threshold | 2 agrees with 0 in 47: one match below it |
    3 32 buckets empty | 4 3's empties, agrees with 3 in 24 of 32: on the threshold with filled = 32 | 5 23 of 32: one below |
    6 an empty signature | 7 n = 0 with 0's sketch: never reported | 8 a copy of 0: identical | 9 0's sketch, another d1: 64 / 64, not identical.
    Every later record is a random earlier one with a random number of buckets redrawn or emptied"""
    rng = np.random.Generator(np.random.PCG64(seed))
    draw = lambda k: rng.integers(0, EMPTY, size=k, dtype=np.uint64).astype(np.uint32)      # never 0xffffffff
    t = np.zeros(max(n, 10), dtype)
    t["n"] = rng.integers(1, 5000, size=len(t))
    t["d0"] = rng.integers(0, 1 << 63, size=len(t), dtype=np.uint64)
    t["d1"] = rng.integers(0, 1 << 63, size=len(t), dtype=np.uint64)
    t["sk"][0] = draw(64)
    for k, keep in ((1, 48), (2, 47)):
        t["sk"][k] = t["sk"][0]
        t["sk"][k][keep:] = (t["sk"][0][keep:] + np.uint32(1)) % np.uint32(EMPTY)      # another value, never 0xffffffff
    t["sk"][3] = draw(64)
    t["sk"][3][1::2] = EMPTY
    for k, keep in ((4, 24), (5, 23)):
        t["sk"][k] = t["sk"][3]
        filled = np.arange(0, 64, 2)
        t["sk"][k][filled[keep:]] = (t["sk"][3][filled[keep:]] + np.uint32(1)) % np.uint32(EMPTY)
    t[6] = (0, 0, 0, 0, [EMPTY] * 64)
    t[7] = (0, 0, 0, 0, t["sk"][0])
    t[8] = t[0]
    t[9] = t[0]
    t["d1"][9] ^= np.uint64(1)
    for k in range(10, len(t)):
        src = int(rng.integers(0, k))
        t["sk"][k] = t["sk"][src]
        change = rng.choice(64, size=int(rng.integers(0, 40)), replace=False)
        t["sk"][k][change] = np.where(rng.random(len(change)) < 0.2, np.uint32(EMPTY), draw(len(change)))
        if rng.random() < 0.1:
            t["n"][k], t["d0"][k], t["d1"][k] = t["n"][src], t["d0"][src], t["d1"][src]
    return t[:n].copy()


def other_table(A, seed: int):
    """a second table for the two-table mode, of another length: most of A backwards (so that pairs exist, identical ones among them) between
    records of a foreign table"""
    F = pair_table(12, seed, A.dtype)
    return np.concatenate([F[:5], A[::-1][: len(A) * 2 // 3 + 1], F[5:]])


def brute_pairs(A, B, thr64: int, pair_dtype):
    """every reported pair by the definition, over whole tables at once -> records sorted by (a, b)"""
    self_mode = B is None
    if self_mode:
        B = A
    eq = (A["sk"][:, None, :] == B["sk"][None, :, :]).sum(-1)
    E = ((A["sk"] == EMPTY)[:, None, :] & (B["sk"] == EMPTY)[None, :, :]).sum(-1)
    match, filled = eq - E, 64 - E
    ok = (A["n"] > 0)[:, None] & (B["n"] > 0)[None, :] & (filled > 0) & (match * 64 >= thr64 * filled)
    if self_mode:
        ok &= np.arange(len(A))[:, None] < np.arange(len(B))[None, :]
    a, b = np.nonzero(ok)                            # row-major: ascending (a, b)
    out = np.zeros(len(a), pair_dtype)
    out["a"], out["b"], out["match"], out["filled"] = a, b, match[a, b], filled[a, b]
    out["flags"] = ((A["n"][a] == B["n"][b]) & (A["d0"][a] == B["d0"][b]) & (A["d1"][a] == B["d1"][b])).astype(np.uint16)
    return out
