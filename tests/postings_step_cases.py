"""Hand-made posting lists for the walks over a list that the index operations share (remove, split, permute, rebase; device and host),
independent of any build.  The walks take a list 256 bytes per step, four bytes per lane, and the subtle parts of the byte format sit at the step
edge: a varint that straddles it, lane 63's window (which ends in the next step's first word) and a list that ends in the middle of a word.  The
lists here put those cases at the edge on purpose:

  straddle   a head, one-byte deltas up to byte P, ONE delta of w bytes starting at byte P, a dozen one-byte deltas; w in 2 .. 4 and P in
             252 .. 256, so every straddle of the edge (P = 256 - w + 1 .. 255) and its aligned neighbours (252, 256)
  exact      lists of exactly 255 .. 257 and 511 .. 513 bytes (the end on a word edge, on a step edge, one byte past either); the last delta
             takes two bytes
  multi      three steps with a wide delta on both edges

Deltas of five bytes would need more than 2^28 structures per index and are left out here, because remove and permute allocate per structure;
tests/merge_cases.py reaches them (merge, load, slice and verify allocate nothing per structure) and merges the results of the operations
here with a part that follows them, which shows the last ids they carry.  Heads of five bytes are there (first_id = 2^28), also
where split writes the head of a piece.  The wide index holds every list over just above 2^21 structures (the four-byte delta needs them); the
narrow one leaves the four-byte deltas out and is small enough for the bitmap of k_permute.hip to stay in LDS.  Expected results come from
Python alone: decode, transform, delta, LEB128 (the codec of tests/rebase_cases.py)."""
import functools

import numpy as np

from tests.rebase_cases import decode, encode, varint  # noqa: F401  (re-exported for the tests)

WIDTHS = (2, 3, 4)
WIDE_DELTA = {2: 1500, 3: 20000, 4: (1 << 21) + 5}      # >= 128, >= 16384, >= 2^21; every one lands past RUN_END
STARTS = (252, 253, 254, 255, 256)
EXACT_LENGTHS = (255, 256, 257, 511, 512, 513)
MULTI = ((4, 3), (3, 2), (2, 4))                        # widths on the first and the second edge (a list has room for one four-byte delta)
FIRST_IDS = (0, 1 << 28)
N_WIDE = (1 << 21) + (1 << 16)
N_NARROW = 1 << 16
HEAD = 3                                                # local id of every list's head
TAIL = 12
RUN_END = 1000                                          # the one-byte run before the first wide delta ends below first_id + RUN_END ...
RUN_MID = 200                                           # ... and passes first_id + RUN_MID (deltas of 1 .. 3 over at least 246 bytes)
SORT_BYTES_LOW = 128                                    # FDGPU_PERM_SORT_BYTES: every list here then takes the bitmap kernel
LDS_BITS_LOW = 4096                                     # FDGPU_PERM_LDS_BITS: below both indexes' structures, every bitmap then a global slab


def n_structures(narrow: bool) -> int:
    return N_NARROW if narrow else N_WIDE


def _build(first_id: int, seed: int, plan):
    """plan: ("run_to", byte) one-byte deltas up to that byte, ("wide", w) one delta of w bytes, ("run", n) n one-byte deltas
    -> (ids, [(element index, start byte, w) of every wide delta])"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids, pos, wide = [first_id + HEAD], len(varint(first_id + HEAD)), []
    for what, arg in plan:
        if what == "wide":
            wide.append((len(ids), pos, arg))
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
    for _, p, w in wide:      # the wide varint starts at byte p and takes w bytes
        assert blob[p - 1] < 0x80 and all(b >= 0x80 for b in blob[p:p + w - 1]) and blob[p + w - 1] < 0x80
    return ids, wide


@functools.lru_cache(maxsize=None)
def lists_of(first_id: int, narrow: bool):
    """[(name, ids, wide)] in hash order; list k gets hash 3 k + 1"""
    out = []
    for w in WIDTHS:
        for p in STARTS:
            out.append((f"straddle_w{w}_p{p}",) + _build(first_id, 100 * w + p, [("run_to", p), ("wide", w), ("run", TAIL)]))
    for n in EXACT_LENGTHS:
        out.append((f"exact_{n}",) + _build(first_id, 5000 + n, [("run_to", n - 2), ("wide", 2)]))
    for w1, w2 in MULTI:
        out.append((f"multi_w{w1}_w{w2}",) + _build(first_id, 7000 + 10 * w1 + w2, [("run_to", 255), ("wide", w1), ("run_to", 513 - w2), ("wide", w2), ("run", TAIL)]))
    if narrow:
        out = [e for e in out if all(w < 4 for _, _, w in e[2])]
    n = n_structures(narrow)
    assert all(first_id <= ids[0] and ids[-1] < first_id + n and all(a < b for a, b in zip(ids, ids[1:])) for _, ids, _ in out)
    return out


def hashes_of(n: int):
    return (3 * np.arange(n) + 1).astype(np.uint32)


def pack(id_lists, hashes):
    """the non-empty lists with their hashes -> (value, hashes, offsets)"""
    kept = [(encode(l), h) for l, h in zip(id_lists, hashes) if l]
    off = np.concatenate([[0], np.cumsum([len(b) for b, _ in kept])]).astype(np.uint64)
    return np.frombuffer(b"".join(b for b, _ in kept), np.uint8).copy(), np.array([h for _, h in kept], np.uint32), off


@functools.lru_cache(maxsize=None)
def source(first_id: int, narrow: bool):
    """(value, hashes, offsets) of the hand-made index, computed once per process: callers leave the arrays as they are"""
    ls = lists_of(first_id, narrow)
    return pack([ids for _, ids, _ in ls], hashes_of(len(ls)))


def _decoded(first_id: int, narrow: bool):
    """the lists decoded from their own bytes again, so that no expectation rests on _build"""
    ls = lists_of(first_id, narrow)
    return [decode(encode(ids)) for _, ids, _ in ls], hashes_of(len(ls))


# ---- remove
@functools.lru_cache(maxsize=None)
def keep_mask(first_id: int, kind: str):
    """around_wide: of every list, the id before and the id behind each wide delta are dropped (RE-ENCODE: a removed id inside the list);
    below_heads: only the ids below every head (RE-BASE: the head alone changes)"""
    keep = np.ones(N_WIDE, np.uint8)
    if kind == "below_heads":
        keep[:HEAD] = 0
    else:
        for _, ids, wide in lists_of(first_id, False):
            for k, _, _ in wide:
                keep[ids[k - 1] - first_id] = 0
                if k + 1 < len(ids):
                    keep[ids[k + 1] - first_id] = 0
    keep.setflags(write=False)
    return keep


@functools.lru_cache(maxsize=None)
def removed(first_id: int, kind: str):
    lists, hashes = _decoded(first_id, False)
    keep = keep_mask(first_id, kind)
    new = first_id + np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])      # new id of the structure at local position x, if kept
    return pack([[int(new[x - first_id]) for x in l if keep[x - first_id]] for l in lists], hashes)


# ---- split
def bounds(first_id: int):
    """one bound inside the one-byte run of every list, one between the two ids around its first wide delta"""
    return np.array([first_id, first_id + RUN_MID, first_id + RUN_END, first_id + N_WIDE], np.uint64)


@functools.lru_cache(maxsize=None)
def split_parts(first_id: int):
    lists, hashes = _decoded(first_id, False)
    b = [int(x) for x in bounds(first_id)]
    return [pack([[x for x in l if lo <= x < hi] for l in lists], hashes) for lo, hi in zip(b, b[1:])]


# ---- permute
@functools.lru_cache(maxsize=None)
def permutation(narrow: bool, name: str):
    n = n_structures(narrow)
    k = np.arange(n, dtype=np.int64)
    p = {"identity": k, "reversal": n - 1 - k, "shuffle": np.random.Generator(np.random.PCG64(4242)).permutation(n)}[name].astype(np.uint32)
    p.setflags(write=False)
    return p


PERMUTATIONS = ("identity", "reversal", "shuffle")


@functools.lru_cache(maxsize=None)
def permuted(first_id: int, narrow: bool, name: str):
    lists, hashes = _decoded(first_id, narrow)
    p = permutation(narrow, name)
    return pack([sorted(first_id + int(p[x - first_id]) for x in l) for l in lists], hashes)


# ---- rebase: (first_id, new first_id); the heads are first_id + 3: one byte <-> five bytes, and one byte -> two bytes (3 + 125 = 128)
REBASES = ((0, 1 << 28), (1 << 28, 0), (0, 125))


@functools.lru_cache(maxsize=None)
def rebased(first_id: int, new_first_id: int):
    lists, hashes = _decoded(first_id, False)
    return pack([[x - first_id + new_first_id for x in l] for l in lists], hashes)
