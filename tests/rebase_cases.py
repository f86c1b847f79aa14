"""Hand-made posting lists for the index rebase tests (device and host), independent of any build: a pure-Python LEB128 encoder, an index whose
lists start on both sides of every 7-bit varint boundary and whose byte lengths are the ragged-tail and multi-step edges of fd_list_copy, and the
expected result of a shift by decode, shift and re-encode."""
import numpy as np

BASE_HEADS = [0, 127, 128, 16383, 16384, 2097151, 2097152, 268435455, 268435456]      # first ids relative to the index's first_id
LENGTHS = [1, 2, 15, 16, 17, 127, 128, 129, 143, 144, 145, 4200]                      # byte lengths of the lists
N_STRUCTURES = 1 << 29                                                                # every id below stays inside [first_id, first_id + 2^29)
# (declared first_id, shift): with first_id 0 the sources' heads ARE the boundary values (they grow by +1 / +128 / +2^21); with first_id 1 and 2^21
# the results' heads are (shift = -1, -(first_id)), so heads shrink; +128 on 2^21 mixes both in one index
CASES = [(0, 1), (0, 128), (0, 1 << 21), (1, -1), ((1 << 21), -1), ((1 << 21), -(1 << 21)), ((1 << 21), 128), (5, 0)]


def varint(v: int) -> bytes:
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def encode(ids) -> bytes:
    """one posting list: the first id absolute, every later one as the delta from the id before it"""
    return b"".join(varint(x if k == 0 else x - ids[k - 1]) for k, x in enumerate(ids))


def decode(buf: bytes) -> list:
    ids, v, s, run = [], 0, 0, 0
    for b in buf:
        v |= (b & 0x7f) << s
        s += 7
        if not b & 0x80:
            run = v if not ids else run + v
            ids.append(run)
            v, s = 0, 0
    assert s == 0, "a varint leaves its list"
    return ids


def _list_of_length(head: int, n_bytes: int, seed: int):
    """ascending ids from head whose encoding takes exactly n_bytes (None: the head's varint alone is longer): one- and two-byte deltas"""
    room = n_bytes - len(varint(head))
    if room < 0:
        return None
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = [head]
    while room:
        d = int(rng.integers(128, 300)) if room >= 2 and rng.random() < 0.3 else int(rng.integers(1, 128))
        ids.append(ids[-1] + d)
        room -= len(varint(d))
    return ids


def pack(id_lists):
    """id lists in hash order -> (value, hashes, offsets): list k gets hash 3 k + 1; the last list ends on the last value byte"""
    blobs = [encode(l) for l in id_lists]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    return np.frombuffer(b"".join(blobs), np.uint8).copy(), (3 * np.arange(len(blobs)) + 1).astype(np.uint32), off


def make_lists(first_id: int):
    """every (head, length) pair that fits, heads = first_id + BASE_HEADS; the longest lists first, so that the last one is a short one and the
    8-byte window at its start runs past the last value byte"""
    out = []
    for n in sorted(LENGTHS, reverse=True):
        for k, h in enumerate(BASE_HEADS):
            l = _list_of_length(first_id + h, n, 1000 * n + k)
            if l is not None:
                out.append(l)
    assert max(l[-1] for l in out) < first_id + N_STRUCTURES
    return out


def shifted(id_lists, shift: int):
    """decode, shift, re-encode: the lists are decoded from their own bytes again, so the expectation does not rest on make_lists"""
    return pack([[x + shift for x in decode(encode(l))] for l in id_lists])
