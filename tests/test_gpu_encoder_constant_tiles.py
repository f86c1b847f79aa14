"""The posting encoder on the 6-byte elements of the default build's stream (csrc/k_index.hip, codec 2: k_enc_sizes / k_enc_write<uint16_t, true>) where a
tile of 2,048 elements holds ONE value of the u16 plane (hash[23:8]) and where it just does not.  Such a "constant" tile — it lies in one of the forty
buckets hash >> 24, predecessor element included, and the u16 values at its two ends are equal — reads two elements of that plane and not its 4 KB;
every other tile takes the path that loads the plane.  The hand-made streams go through the test-only entry fdgpu_debug_encode_stream_b24 and are
compared byte for byte, no tolerance: hashes, offsets, value bytes and the posting count against the numpy model of tests/encoder_cases.py, the
device checker (ix.verify()), and the per-list last ids through the merge tests/test_gpu_encoder_edges.py uses.

The tile predicate is restated here in numpy (constant_tiles) and every case asserts which of its tiles are constant, so that a case shows what it
is there for: none passes with the constant path never taken, and none of those at a change of the u16 value or of the bucket with it never left.

Case 6 of the plan — a CONSTANT tile of 2,048 five-byte list heads with the low hash byte changing at every element, the tile buffer in LDS full —
cannot exist: a constant tile holds one bucket and one u16 value, so its hashes differ in the low byte alone and it has at most 256 list heads; only
a head can take five bytes (a delta is below 2^24), so the most a constant tile writes is 256 * 5 + 1,792 * 4 = 8,448 of the buffer's 10,240 bytes.
It is split in two, both behind the largest alignment shift (15) and with first_id just below 2^28: the fullest constant tile there is (a head of
five bytes at each of the 255 low bytes the tile in front left over, the elements between them deltas of four and three bytes), and a tile of 2,048
five-byte heads, which fills the buffer and must take the other path (its u16 value changes every 256 elements)."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import oracle
from tests import encoder_cases as ec

pytestmark = pytest.mark.gpu
TILE = ec.TILE


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    faulthandler.dump_traceback_later(600, exit=True)
    c = fd.Context(0)
    yield c
    c.close()
    faulthandler.cancel_dump_traceback_later()


def constant_tiles(h):
    """the encoder's predicate per tile: the predecessor of the tile's first element (element 0 for tile 0) and the tile's last element lie in one
    bucket and carry one u16 value"""
    h = np.asarray(h, np.int64)
    n = len(h)
    t0 = np.arange(0, n, TILE)
    t1 = np.minimum(t0 + TILE, n) - 1
    tp = np.maximum(t0 - 1, 0)
    cst = (h[tp] >> 24 == h[t1] >> 24) & ((h[tp] >> 8) & 0xffff == (h[t1] >> 8) & 0xffff)
    for t in np.flatnonzero(cst):      # what the predicate promises of a sorted stream
        assert len(np.unique(h[tp[t]:t1[t] + 1] >> 8)) == 1
    return [bool(x) for x in cst]


def _fill(prefix, period=37):
    """a sorted stream over per-element (bucket << 16 | u16) values: the low hash byte steps up every `period` elements, so lists start inside tiles and
    (37 divides none of 2,047 .. 2,049, 4,096) run across tile ends; ids per list 0, 0, 3, 3, 6, ... — every second element a repeat -> (hashes, local ids)"""
    prefix = np.asarray(prefix, np.int64)
    n = len(prefix)
    assert n // period < 256 and np.all(prefix[1:] >= prefix[:-1])
    h = prefix << 8 | np.arange(n) // period
    start = np.maximum.accumulate(np.where(np.concatenate([[True], h[1:] != h[:-1]]), np.arange(n), 0))
    return h, (np.arange(n) - start) // 2 * 3


def _encode(ctx, h, loc, first_id):
    import folddisco_amd as fd
    from folddisco_amd import _lib
    h = np.ascontiguousarray(h, np.uint32)
    loc = np.ascontiguousarray(loc, np.uint32)
    out = C.c_void_p()
    ctx.check(ctx.L.fdgpu_debug_encode_stream_b24(ctx.h, h.ctypes.data_as(_lib.u32p), loc.ctypes.data_as(_lib.u32p), len(h), first_id, C.byref(out)))
    return fd.FolddiscoIndex(ctx, out, int(loc.max()) + 1 if len(loc) else 0, first_id)


def _same(name, got, m):
    v, h, o = got
    assert np.array_equal(h, m.hashes), name
    assert np.array_equal(o, m.offsets), name
    assert np.array_equal(v, m.value), name


def _check(ctx, name, h, loc, want_constant, first_id=0, model_check=None):
    import folddisco_amd as fd
    h, loc = np.asarray(h, np.int64), np.asarray(loc, np.int64)
    assert constant_tiles(h) == list(want_constant), (name, constant_tiles(h))
    ids = loc + first_id
    m = ec.Model(h, ids)
    if model_check:
        model_check(m)
    ix = _encode(ctx, h, loc, first_id)
    _same(name, ix.export(), m)
    assert ix.num_postings == m.n_postings, name
    rep = ix.verify()
    assert rep.ok and rep.n_lists == len(m.hashes) and rep.n_postings == m.n_postings, (name, rep)
    S = first_id + ix.n_structures      # last ids: merge with an index that holds structure S in every list
    tail = ec.Model(m.hashes, np.full(len(m.hashes), S, np.uint64).astype(np.uint32))
    ix2 = fd.FolddiscoIndex.load(ctx, tail.hashes, tail.offsets, tail.value, 1, first_id=S)
    merged = fd.FolddiscoIndexSet([ix, ix2]).merge()
    hh = np.concatenate([h, m.hashes]).astype(np.uint64)
    ii = np.concatenate([ids, np.full(len(m.hashes), S)]).astype(np.uint64)
    order = np.argsort((hh << np.uint64(32)) | ii, kind="stable")
    _same(name + " (merged)", merged.export(), ec.Model(hh[order], ii[order]))


B, U = 3, 0x1234      # a bucket and a u16 value somewhere in the middle


def test_one_u16_value_over_three_tiles_and_a_bit(ctx):
    h, loc = _fill(np.full(3 * TILE + 100, B << 16 | U))

    def chk(m):      # list heads inside the tiles, repeats that drop out
        assert m.item_head[1:TILE].sum() > 40 and m.item_head[TILE + 1:2 * TILE].sum() > 40 and (m.item_len == 0).sum() > TILE
    _check(ctx, "one u16 value", h, loc, [True] * 4, model_check=chk)


@pytest.mark.parametrize("x,want", [(TILE - 1, [False, True, True]), (TILE, [True, False, True]), (TILE + 1, [True, False, True])],
                         ids=["at C-1", "at C", "at C+1"])
def test_u16_value_changes_around_a_tile_end(ctx, x, want):
    n = 2 * TILE + 50
    pre = np.where(np.arange(n) < x, B << 16 | U, B << 16 | (U + 1))
    h, loc = _fill(pre)

    def chk(m):
        assert m.item_head[x]
        if x == TILE:      # tile 1 is constant inside itself, its predecessor is not of it
            assert len(np.unique(h[TILE:2 * TILE] >> 8)) == 1 and h[TILE - 1] >> 8 != h[TILE] >> 8
    _check(ctx, f"u16 changes at {x}", h, loc, want, model_check=chk)


@pytest.mark.parametrize("equal_ids", [True, False], ids=["equal ids", "different ids"])
@pytest.mark.parametrize("x,want", [(TILE - 1, [False, True, True]), (TILE, [True, False, True]), (TILE + 1, [True, False, True])],
                         ids=["at C-1", "at C", "at C+1"])
def test_bucket_boundary_with_identical_low_24_hash_bits(ctx, x, want, equal_ids):
    n = 2 * TILE + 50
    pre = np.where(np.arange(n) < x, B << 16 | U, (B + 1) << 16 | U)
    h, loc = _fill(pre)
    assert h[x - 1] & 0xffffff == h[x] & 0xffffff and h[x - 1] >> 24 == B and h[x] >> 24 == B + 1
    lst = h == h[x]      # the list behind the boundary: shifted up so that it starts at the id in front of it, or one above
    assert loc[x] == 0 and loc[x - 1] > 0
    loc = np.where(lst, loc + loc[x - 1] + (0 if equal_ids else 1), loc)

    def chk(m):      # a head although the 24 bits the planes hold repeat, and with the same id in the one run
        assert m.item_head[x] and m.item_len[x] > 0 and (loc[x] == loc[x - 1]) == equal_ids
    _check(ctx, f"bucket boundary at {x}", h, loc, want, model_check=chk)


@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_stream_lengths_with_one_u16_value(ctx, n):
    h, loc = _fill(np.full(n, B << 16 | U))
    _check(ctx, f"n={n}", h, loc, [True] * ((n + TILE - 1) // TILE))      # a constant partial last tile; tile 0, whose predecessor is itself


def test_constant_tile_of_repeats_of_the_previous_tiles_last_element(ctx):
    h, loc = _fill(np.full(TILE, B << 16 | U))
    h = np.concatenate([h, np.full(TILE, h[-1]), [h[-1], h[-1] + 1]])
    loc = np.concatenate([loc, np.full(TILE, loc[-1]), [loc[-1] + 70000, 3]])

    def chk(m):      # tile 1 holds no posting and no head
        assert (m.item_len[TILE:2 * TILE] == 0).all() and not m.item_head[TILE:2 * TILE].any() and m.item_len[TILE - 1] > 0 and m.item_len[2 * TILE] > 0
    _check(ctx, "a tile of repeats", h, loc, [True] * 3, model_check=chk)


FIRST_ID_28 = (1 << 28) - 5      # the first five local ids are four-byte heads, every other head takes five


def _tile0_shift15():
    """tile 0: one list whose bytes end at 15 mod 16 (its head at local id 10: five bytes, then one-byte deltas, then repeats of its last id)"""
    m = 2027      # 5 + (m - 1) = 2,031 = 15 mod 16
    return np.full(TILE, (B << 16 | U) << 8), np.concatenate([10 + np.arange(m), np.full(TILE - m, 10 + m - 1)])


def test_fullest_constant_tile_behind_the_largest_alignment_shift(ctx):
    h0, l0 = _tile0_shift15()
    j = np.arange(TILE)
    low = 1 + j * 255 // TILE      # every low byte tile 0's list left: 255 lists of 8 or 9 elements
    start = np.maximum.accumulate(np.where(np.concatenate([[True], low[1:] != low[:-1]]), j, 0))
    k = j - start
    l1 = np.where(k < 8, 100 + k * (1 << 21), (1 << 24) - 1)      # five-byte head, four-byte deltas (2^21), a ninth element of three
    h = np.concatenate([h0, h0[0] + low, [h0[0] + 0x100, h0[0] + 0x100]])
    loc = np.concatenate([l0, l1, [7, 9]])

    def chk(m):
        t1 = slice(TILE, 2 * TILE)
        assert int(m.offsets[1]) % 16 == 15 and m.item_head[t1].sum() == 255 and (m.item_len[t1][m.item_head[t1]] == 5).all()
        assert (m.item_len[t1] == 4).sum() >= 255 * 7 and int(m.item_len[t1].sum()) > 8000
    _check(ctx, "fullest constant tile", h, loc, [True, True, False], first_id=FIRST_ID_28, model_check=chk)


def test_tile_of_five_byte_heads_behind_the_largest_alignment_shift_is_not_constant(ctx):
    h0, l0 = _tile0_shift15()
    rng = np.random.default_rng(53)
    j = np.arange(TILE + 70)
    h1 = ((B << 16 | (U + 1 + j // 256)) << 8) | j % 256      # the low byte changes at every element, the u16 value every 256
    h = np.concatenate([h0, h1])
    loc = np.concatenate([l0, rng.integers(5, 1 << 24, len(j))])

    def chk(m):      # 10,240 bytes behind the largest shift: the tile buffer in LDS full
        assert (m.item_len[TILE:2 * TILE] == 5).all() and m.item_head[TILE:2 * TILE].all() and int(m.offsets[1]) % 16 == 15
    _check(ctx, "2048 five-byte heads", h, loc, [True, False, False], first_id=FIRST_ID_28, model_check=chk)


def test_forty_buckets_of_which_the_first_and_the_last_hold_elements(ctx):
    pre = np.concatenate([np.full(TILE + 100, 0 << 16 | U), np.full(2 * TILE, 39 << 16 | 7)])
    h, loc = _fill(pre)
    assert set(h >> 24) == {0, 39}
    _check(ctx, "buckets 0 and 39", h, loc, [True, False, True, True])


# ---- through a real build, sort included
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _chain(rng, n):
    ca = np.cumsum(_unit(rng, n) * 3.8, axis=0) + rng.uniform(-30.0, 30.0, size=3)
    return dict(n=(ca + 1.46 * _unit(rng, n)).astype(np.float32), ca=ca.astype(np.float32), cb=(ca + 1.53 * _unit(rng, n)).astype(np.float32),
                aa=rng.integers(0, 20, size=n).astype(np.uint8), ok=np.ones(n, np.uint8))


def _oracle_index(items):
    """-> (the oracle's index over the items with ids from 0, their hash lists concatenated, the CSR offsets)"""
    structs = [oracle.structure_from_packed(s["n"], s["ca"], s["cb"], s["aa"], cb_ok=s["ok"]) for s in items]
    h, off = oracle.hash_batch(structs)
    off = off.astype(np.int64)
    L = oracle.lib()
    ix = L.fdo_index_new(30)
    for fn in (L.fdo_index_count_single_entry, L.fdo_index_add_single_entry):
        for s in range(len(off) - 1):
            for x in h[off[s]:off[s + 1]]:
                fn(ix, int(x), s)
        if fn is L.fdo_index_count_single_entry:
            L.fdo_index_allocate_entries(ix)
    L.fdo_index_finish(ix)
    return oracle.OIndex(ix), h, off


def _upload(ctx, items):
    import folddisco_amd as fd
    res_off = np.concatenate([[0], np.cumsum([len(s["aa"]) for s in items])]).astype(np.uint64)
    cat = lambda k: np.concatenate([s[k] for s in items])
    return ctx.upload(fd.PackedStructures(res_off, cat("n"), cat("ca"), cat("cb"), cat("aa"), cat("ok")))


def test_real_build_of_repeated_structures(ctx, monkeypatch):
    import folddisco_amd as fd
    for k in ("FDGPU_MSD", "FDGPU_IDS32"):
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(7855)      # a seed at which the oracle gives every structure its six hashes and the stream the share of constant tiles asserted below
    one = _chain(rng, 3)
    own = [_chain(rng, 3) for _ in range(200)]
    items = [own[s // 21] if s % 21 == 20 else one for s in range(4200)]      # 4,000 copies, every 21st structure one of its own
    oix, h, off = _oracle_index(items)
    oown, _, _ = _oracle_index(own)
    # the stream the encoder gets: every structure's hashes with its id, sorted.  The oracle's lists are per structure sorted and unique; with
    # six of them for every structure (one per ordered residue pair) no pair was dropped or repeated, so they ARE the build's keys
    assert len(h) == 6 * len(items) and int(h.max()) < 1 << 30 and int(h.max()) >> 24 < 40
    ids = np.repeat(np.arange(len(items)), np.diff(off))
    stream = np.sort(h.astype(np.int64) << 32 | ids) >> 32
    cst = constant_tiles(stream)
    assert len(cst) >= 12 and 2 * sum(cst) >= len(cst) and not all(cst), cst
    big, small = _upload(ctx, items), _upload(ctx, own)
    for batch, want in ((big, oix), (small, oown), (big, oix)):      # one context: the workspace of the one build is what the next one finds
        ix = fd.FolddiscoIndex.build(ctx, batch)
        v, hh, o = ix.export()
        assert np.array_equal(hh, want.hashes()) and np.array_equal(o, want.offsets()) and np.array_equal(v, want.values())
        assert ix.verify().ok
