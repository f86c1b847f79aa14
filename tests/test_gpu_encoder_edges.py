"""The posting encoder (csrc/k_index.hip: k_enc_sizes + k_enc_write) on streams that proteins never produce, through the test-only entry
fdgpu_debug_encode_stream: hashes, offsets, value bytes and the posting count against the numpy model of tests/encoder_cases.py (itself equal to the
oracle, tests/test_encoder_cases_host.py), byte for byte, no tolerance; every index also passes the device checker (fdgpu_index_verify).  The
checker does not look at the per-list last ids the write pass leaves for later merges, so they are checked through a merge: one more posting behind
every list is encoded as the delta from that list's last id.

The cases (tests/encoder_cases.py asserts on the model that each shows what it is there for): stream lengths around one and two tiles of 2,048
elements; list heads and deltas at every varint length boundary at each of a thread's eight item positions, at the last item of a thread, a
wavefront and a tile and at the first of the next; the second tile starting at every byte offset mod 16; a tile of 2,048 heads; a tile of 2,048
five-byte varints behind the largest alignment shift (the tile buffer in LDS full); one list over three tiles; repeats across thread, wavefront
and tile boundaries and a tile that holds nothing else.  The 6-byte stream encodings, which the entry does not reach, get one build of a few
hundred tiny structures with first_id just below 2^21 and 2^28 in all three forms of the build, against the oracle's index with the same ids."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import oracle
from tests import encoder_cases as ec

pytestmark = pytest.mark.gpu
CASES = ec.all_cases()


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    faulthandler.dump_traceback_later(600, exit=True)
    c = fd.Context(0)
    yield c
    c.close()
    faulthandler.cancel_dump_traceback_later()


def _encode(ctx, h, i):
    import folddisco_amd as fd
    from folddisco_amd import _lib
    h = np.ascontiguousarray(h, np.uint32)
    i = np.ascontiguousarray(i, np.uint32)
    out = C.c_void_p()
    ctx.check(ctx.L.fdgpu_debug_encode_stream(ctx.h, h.ctypes.data_as(_lib.u32p), i.ctypes.data_as(_lib.u32p), len(h), C.byref(out)))
    return fd.FolddiscoIndex(ctx, out, int(i.max()) + 1 if len(i) else 0)


def _same(name, got, m):
    v, h, o = got
    assert np.array_equal(h, m.hashes), name
    assert np.array_equal(o, m.offsets), name
    assert np.array_equal(v, m.value), name


def _check(ctx, name):
    import folddisco_amd as fd
    h, i, _ = CASES[name]
    m = ec.Model(h, i)
    ix = _encode(ctx, h, i)
    _same(name, ix.export(), m)
    assert ix.num_postings == m.n_postings, name
    rep = ix.verify()
    assert rep.ok and rep.n_lists == len(m.hashes) and rep.n_postings == m.n_postings, (name, rep)
    S = m.n_structures
    if S + 1 <= 0xffffffff:      # last ids: merge with an index that holds structure S in every list
        tail = ec.Model(m.hashes, np.full(len(m.hashes), S, np.uint64).astype(np.uint32))
        ix2 = fd.FolddiscoIndex.load(ctx, tail.hashes, tail.offsets, tail.value, 1, first_id=S)
        merged = fd.FolddiscoIndexSet([ix, ix2]).merge()
        hh = np.concatenate([h, m.hashes]).astype(np.uint64)
        ii = np.concatenate([i, np.full(len(m.hashes), S)]).astype(np.uint64)
        order = np.argsort((hh << np.uint64(32)) | ii, kind="stable")
        _same(name + " (merged)", merged.export(), ec.Model(hh[order], ii[order]))


@pytest.mark.parametrize("n", [1, 2, 2047, 2048, 2049, 4097])
def test_stream_lengths(ctx, n):
    _check(ctx, f"n={n}")


@pytest.mark.parametrize("v", ec.BOUNDARY_VALUES, ids=[hex(v) for v in ec.BOUNDARY_VALUES])
def test_length_boundaries_at_every_item_position_and_across_thread_wave_and_tile(ctx, v):
    for kind in ("head", "delta"):
        for tag in ("A", "B"):
            _check(ctx, f"{kind} {v:#x} {tag}")


def test_second_tile_at_every_byte_offset(ctx):
    for k in range(16):
        _check(ctx, f"tile 1 at byte {k} mod 16")


@pytest.mark.parametrize("name", ["2048 heads", "2048 five-byte varints", "one list over three tiles", "duplicate runs, tail 0", "duplicate runs, tail 5",
                                  "a tile of repeats of the previous tile's last element"])
def test_full_tiles_long_lists_and_repeats(ctx, name):
    _check(ctx, name)


def test_every_case_ran():
    ran = {f"n={n}" for n in (1, 2, 2047, 2048, 2049, 4097)} | {f"{k} {v:#x} {t}" for v in ec.BOUNDARY_VALUES for k in ("head", "delta") for t in "AB"}
    ran |= {f"tile 1 at byte {k} mod 16" for k in range(16)}
    ran |= {"2048 heads", "2048 five-byte varints", "one list over three tiles", "duplicate runs, tail 0", "duplicate runs, tail 5",
            "a tile of repeats of the previous tile's last element"}
    assert ran == set(CASES)


# ---- the 6-byte stream encodings (k_enc_write<uint16_t, false> and <uint16_t, true>) and the 8-byte one through a whole build
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _chain(rng, n):
    ca = np.cumsum(_unit(rng, n) * 3.8, axis=0) + rng.uniform(-30.0, 30.0, size=3)
    return dict(n=(ca + 1.46 * _unit(rng, n)).astype(np.float32), ca=ca.astype(np.float32), cb=(ca + 1.53 * _unit(rng, n)).astype(np.float32),
                aa=rng.integers(0, 20, size=n).astype(np.uint8), ok=np.ones(n, np.uint8))


@pytest.fixture(scope="module")
def tiny():
    """300 structures of two to four residues, four geometries that repeat (lists of ~75 consecutive-ish ids) and a dozen of their own
    -> (items, per-structure sorted-unique hash lists of the oracle as CSR)"""
    rng = np.random.default_rng(7301)
    shared = [_chain(rng, 2 + k % 3) for k in range(4)]
    items = [shared[s % 4] if s % 25 else _chain(rng, 2 + s % 3) for s in range(300)]
    structs = [oracle.structure_from_packed(s["n"], s["ca"], s["cb"], s["aa"], cb_ok=s["ok"]) for s in items]
    h, off = oracle.hash_batch(structs)
    return items, h, off.astype(np.int64)


def _oracle_index_with_ids(h, off, first_id):
    L = oracle.lib()
    ix = L.fdo_index_new(30)
    for fn in (L.fdo_index_count_single_entry, L.fdo_index_add_single_entry):
        for s in range(len(off) - 1):
            for x in h[off[s]:off[s + 1]]:
                fn(ix, int(x), first_id + s)
        if fn is L.fdo_index_count_single_entry:
            L.fdo_index_allocate_entries(ix)
    L.fdo_index_finish(ix)
    return oracle.OIndex(ix)


@pytest.mark.parametrize("first_id", [(1 << 21) - 150, (1 << 28) - 150], ids=["below 2^21", "below 2^28"])
def test_six_byte_stream_encodings_with_heads_across_a_length_boundary(ctx, monkeypatch, tiny, first_id):
    import folddisco_amd as fd
    items, h, off = tiny
    oix = _oracle_index_with_ids(h, off, first_id)
    heads = np.array([int(oix.entries(int(x))[0]) for x in oix.hashes()])
    bound = first_id + 150
    assert (heads < bound).any() and (heads >= bound).any() and int(h.max()) < 1 << 30      # heads of both lengths; every hash fits the 6-byte element
    assert int(ec.varint_len(bound - 1)) + 1 == int(ec.varint_len(bound))
    res_off = np.concatenate([[0], np.cumsum([len(s["aa"]) for s in items])]).astype(np.uint64)
    cat = lambda k: np.concatenate([s[k] for s in items])
    batch = ctx.upload(fd.PackedStructures(res_off, cat("n"), cat("ca"), cat("cb"), cat("aa"), cat("ok")))
    for form in ({}, {"FDGPU_MSD": "0"}, {"FDGPU_IDS32": "1"}):
        for k in ("FDGPU_MSD", "FDGPU_IDS32"):
            monkeypatch.delenv(k, raising=False)
        for k, v in form.items():
            monkeypatch.setenv(k, v)
        ix = fd.FolddiscoIndex.build(ctx, batch, first_id=first_id)
        v, hh, o = ix.export()
        assert np.array_equal(hh, oix.hashes()), form
        assert np.array_equal(o, oix.offsets()), form
        assert np.array_equal(v, oix.values()), form
        assert ix.verify().ok, form
    for k in ("FDGPU_MSD", "FDGPU_IDS32"):
        monkeypatch.delenv(k, raising=False)
