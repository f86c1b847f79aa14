"""Hand-made posting lists for the index reorder tests (device and host), independent of any build: an index over N structures whose lists have
the id counts and byte lengths at which the permute kernels change their path, a set of permutations, and the expected result by Python alone
(decode, map, sorted, encode).  The varint codec and the packer are those of tests/rebase_cases.py."""
import functools

import numpy as np

from tests.rebase_cases import decode, encode, pack, varint  # noqa: F401  (re-exported for the tests)

N = 20000                                    # structures; every list holds ids of [first_id, first_id + N)
FIRST_IDS = [0, 2097000]                     # 2,097,000: heads and deltas on both sides of 2^21 = 2,097,152 (three- and four-byte varints)
# ids per list: the wave scan's and the 64-ids-per-step re-delta's edges (63 / 64 / 65), one 256-byte decode step and more (255 / 256 / 257
# ids are 255 .. 514 bytes), the powers of two of the bitonic network (1023 / 1024 / 1025)
ID_COUNTS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
# byte lengths per list: the class boundary of csrc/k_permute.hip (PM_SORT_BYTES = 2048: one below, the boundary, one above), the same around
# the value the tests lower it to (SORT_BYTES_LOW), and the decode step (256 bytes; 2048 is also the eight steps of the bitmap kernel)
SORT_BYTES = 2048
SORT_BYTES_LOW = 512
LDS_BITS_LOW = 4096                          # below N: with FDGPU_PERM_LDS_BITS at this value every bitmap list takes a global-memory slab
BYTE_LENGTHS = [255, 256, 257, SORT_BYTES_LOW - 1, SORT_BYTES_LOW, SORT_BYTES_LOW + 1, SORT_BYTES - 1, SORT_BYTES, SORT_BYTES + 1, 4097]


def _ids_by_count(first_id: int, count: int, seed: int):
    """count ascending ids of [first_id, first_id + N): a random head, then a seeded mix of one-byte deltas and, where the range has room for
    them, two-byte ones (128 .. 300)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if count == 1:
        return [first_id + int(rng.integers(0, N))]
    room = N - 1                                                   # head + sum of the deltas <= N - 1
    n2 = min((count - 1) // 8, (room - (count - 1)) // 600)         # two-byte deltas: about every eighth, while 300 each leave half the room
    n1 = count - 1 - n2
    hi = max(1, min(127, (room - 300 * n2) // max(n1, 1) - 1))      # one-byte deltas 1 .. hi: their sum stays inside what is left
    deltas = [int(x) for x in rng.integers(128, 301, n2)] + [int(x) for x in rng.integers(1, hi + 1, n1)]
    rng.shuffle(deltas)
    head = int(rng.integers(0, room - sum(deltas) + 1))
    ids = first_id + head + np.concatenate([[0], np.cumsum(deltas)])
    return [int(x) for x in ids]


def _ids_by_bytes(first_id: int, n_bytes: int, seed: int):
    """ascending ids of [first_id, first_id + N) whose encoding takes exactly n_bytes: 40 two-byte deltas among one-byte ones of 1 .. 4"""
    rng = np.random.Generator(np.random.PCG64(seed))
    head = first_id + int(rng.integers(0, 100))
    room = n_bytes - len(varint(head))
    n2 = min(40, room // 4)
    n1 = room - 2 * n2
    deltas = [int(x) for x in rng.integers(128, 200, n2)] + [int(x) for x in rng.integers(1, 5, n1)]
    rng.shuffle(deltas)
    ids = [int(x) for x in head + np.concatenate([[0], np.cumsum(deltas)])]
    assert len(encode(ids)) == n_bytes and ids[-1] < first_id + N, (n_bytes, ids[-1])
    return ids


def make_lists(first_id: int):
    """the hand-made index: every id count, every byte length, the list of all N ids, and a last list of one byte (for first_id 0) or of one id
    that ends on the last value byte"""
    out = [_ids_by_count(first_id, c, 7000 + c) for c in ID_COUNTS]
    out += [_ids_by_bytes(first_id, b, 9000 + b) for b in BYTE_LENGTHS]
    out.append(list(range(first_id, first_id + N)))
    out.append([first_id + 5])
    assert all(first_id <= l[0] and l[-1] < first_id + N and all(a < b for a, b in zip(l, l[1:])) for l in out)
    return out


def permutations():
    """name -> new_id (new_id[k] = new position of the structure at position k)"""
    k = np.arange(N, dtype=np.int64)
    swap = k.copy()
    swap[127], swap[128] = 128, 127
    return {
        "identity": k.astype(np.uint32),
        "reversal": (N - 1 - k).astype(np.uint32),
        "random": np.random.Generator(np.random.PCG64(4242)).permutation(N).astype(np.uint32),
        "swap127_128": swap.astype(np.uint32),
        "rotate1": ((k + 1) % N).astype(np.uint32),
        "evens_then_odds": np.where(k % 2 == 0, k // 2, (N + 1) // 2 + k // 2).astype(np.uint32),
    }


def inverse(new_id):
    inv = np.empty(len(new_id), np.uint32)
    inv[np.asarray(new_id, dtype=np.int64)] = np.arange(len(new_id), dtype=np.uint32)
    return inv


def permuted(id_lists, new_id, first_id: int):
    """decode, map, sorted, encode: the lists are decoded from their own bytes again, so the expectation does not rest on make_lists"""
    p = [int(x) for x in new_id]
    return pack([sorted(first_id + p[x - first_id] for x in decode(encode(l))) for l in id_lists])


@functools.lru_cache(maxsize=None)
def lists_of(first_id: int):
    return make_lists(first_id)


@functools.lru_cache(maxsize=None)
def case(first_id: int, name: str):
    """(id lists, the packed source, the packed expectation) of one case, computed once per process: callers leave the arrays as they are"""
    lists = lists_of(first_id)
    return lists, pack(lists), permuted(lists, permutations()[name], first_id)
