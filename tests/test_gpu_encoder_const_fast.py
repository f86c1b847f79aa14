"""The posting encoder's fast path for a full constant tile behind tile 0 (csrc/k_index.hip: enc_classify_const; the rule per element is
fd_const_classify of csrc/fd_postings.h).  In such a tile every element shares bucket and hash[23:8] with its predecessor, so the kernels tell heads, repeats and deltas from the u32
key word (hash[7:0] << 24 | local id) alone, and make what a head needs only in a wavefront that holds one.

Hand-made streams of a few tiles of 2,048 go through the test-only entry fdgpu_debug_encode_stream_b24 and are checked as
tests/test_gpu_encoder_constant_tiles.py checks its own (its _check): byte-exact against tests/encoder_cases.Model, ix.verify(), the last ids
through the merge.  Every case restates the path predicate in numpy (fast_tiles) and asserts on the model that it shows what it is there for.

Two figures differ from the plan of the cases.  "A constant tile with 256 heads" exists only as tile 0: a tile on the fast path shares its u16
value with its predecessor, whose low hash byte is at least 0, so 255 low bytes are left for its heads; both are here (256 in tile 0, which goes
the general way, 255 in tile 1).  And the sequence general / fast / general / fast / partial takes four full tiles and a few elements, not three."""
import faulthandler

import numpy as np
import pytest

from tests import encoder_cases as ec
from tests.test_gpu_encoder_constant_tiles import B, U, _check, constant_tiles

pytestmark = pytest.mark.gpu
TILE, WAVE, ITEMS = ec.TILE, ec.WAVE, ec.ITEMS
H0 = (B << 16 | U) << 8      # low hash byte 0 of the bucket and u16 value the constant tiles hold

# positions in tile 1: each of a thread's eight item positions (eight threads of wavefront 0; the first is also the first item of a thread), the
# first item of a wavefront (its predecessor comes from memory) and of tile 1 (its predecessor lies in tile 0)
ITEM_POS = tuple(TILE + 8 * (3 + 2 * j) + j for j in range(ITEMS))
POS = (TILE,) + ITEM_POS + (TILE + WAVE,)


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    faulthandler.dump_traceback_later(600, exit=True)
    c = fd.Context(0)
    yield c
    c.close()
    faulthandler.cancel_dump_traceback_later()


def fast_tiles(h):
    """the fast path's predicate per tile: constant, full, not tile 0"""
    n = len(h)
    return [bool(c) and t > 0 and (t + 1) * TILE <= n for t, c in enumerate(constant_tiles(h))]


def words(h, loc):
    return (np.asarray(h, np.int64) & 0xff) << 24 | np.asarray(loc, np.int64)


def check(ctx, name, h, loc, want_fast, first_id=0, model_check=None):
    h, loc = np.asarray(h, np.int64), np.asarray(loc, np.int64)
    assert [p % ITEMS for p in ITEM_POS] == list(range(ITEMS)) and (TILE + WAVE) % WAVE == 0
    assert fast_tiles(h) == list(want_fast), (name, fast_tiles(h))
    _check(ctx, name, h, loc, constant_tiles(h), first_id=first_id, model_check=model_check)


def lists_from_low(low, start_id=5, step=3, rep=1):
    """ids per list (a run of one value of low): start_id, start_id + step, ..., each rep times"""
    low = np.asarray(low, np.int64)
    n = len(low)
    start = np.maximum.accumulate(np.where(np.concatenate([[True], low[1:] != low[:-1]]), np.arange(n), 0))
    return start_id + (np.arange(n) - start) // rep * step


def stepped_low(n, positions):
    """low hash byte: one more at every position -> a list head there"""
    low = np.zeros(n, np.int64)
    for p in positions:
        low[p:] += 1
    return low


N3 = 2 * TILE + 5      # tile 0 (general), tile 1 (fast), a partial tile 2 (general)


def test_head_with_a_smaller_id_than_its_predecessor(ctx):
    low = stepped_low(N3, POS)
    h, loc = H0 + low, lists_from_low(low)
    w = words(h, loc)

    def chk(m):
        for p in POS:      # a head, and the subtraction of the words looks like a delta
            assert m.item_head[p] and loc[p] < loc[p - 1] and 0 < w[p] - w[p - 1] < 1 << 24, p
        assert not m.item_head[TILE + 2 * WAVE:2 * TILE].any()      # wavefronts 2 and 3 of tile 1 hold no head
    check(ctx, "heads with smaller ids", h, loc, [False, True, False], model_check=chk)


def test_head_with_the_id_of_its_predecessor(ctx):
    low = stepped_low(N3, POS)
    h = H0 + low
    inc = np.ones(N3, np.int64)
    inc[list(POS)] = 0
    loc = 7 + np.cumsum(inc)      # ascending over the whole stream, one more at every element but the heads: each has the id in front of it

    def chk(m):
        for p in POS:
            assert m.item_head[p] and m.item_len[p] == 2 and loc[p] == loc[p - 1], p
        assert (m.item_len == 0).sum() == 0      # equal words apart from the top byte, and no repeat
    check(ctx, "heads with equal ids", h, loc, [False, True, False], model_check=chk)


def test_repeat_of_the_predecessor(ctx):
    low = np.arange(N3) // 700
    h = H0 + low
    inc = np.full(N3, 3, np.int64)
    inc[list(POS)] = 0      # the element repeats the one in front of it; the list goes on from there
    loc = 5 + np.cumsum(inc)
    assert all(low[p] == low[p - 1] for p in POS)

    def chk(m):
        for p in POS:
            assert m.item_len[p] == 0 and not m.item_head[p] and m.item_len[p - 1] > 0 and m.item_len[p + 1] > 0, p
        assert (m.item_len == 0).sum() == len(POS)
    check(ctx, "repeats", h, loc, [False, True, False], model_check=chk)


@pytest.mark.parametrize("d", [0x7f, 0x80, 0x3fff, 0x4000, 0x1fffff, 0x200000, (1 << 24) - 1], ids=hex)
def test_delta_at_a_varint_boundary(ctx, d):
    low = stepped_low(N3, [p - 1 for p in POS])      # a head of id 0 in front of each position, the delta at it
    h = H0 + low
    loc = lists_from_low(low, start_id=1, step=1)
    for p in POS:
        loc[p - 1] = 0
        loc[p] = d
        q = p + 1
        while q < N3 and low[q] == low[p]:      # the rest of the list: repeats of d
            loc[q] = d
            q += 1

    def chk(m):
        for p in POS:
            assert int(m.item_delta[p]) == d and int(m.item_len[p]) == int(ec.varint_len(d)) and not m.item_head[p] and m.item_head[p - 1], p
    check(ctx, f"delta {d:#x}", h, loc, [False, True, False], model_check=chk)


def test_constant_tile_with_255_heads_and_tile_0_with_256(ctx):
    low1 = 1 + np.arange(TILE) * 255 // TILE      # tile 1: every low byte that tile 0 (low byte 0) leaves, eight or nine elements each
    low = np.concatenate([np.zeros(TILE, np.int64), low1, [255, 255]])
    h, loc = H0 + low, lists_from_low(low, step=1000)

    def chk(m):
        assert m.item_head[TILE:2 * TILE].sum() == 255 and m.item_head[TILE] and (m.item_len[TILE:2 * TILE] == 2).sum() > 1500
    check(ctx, "255 heads", h, loc, [False, True, False], model_check=chk)
    low = np.concatenate([np.arange(TILE) // 8, np.full(TILE + 3, 255)])      # tile 0: 256 heads, constant, the general way; tile 1 goes on
    h, loc = H0 + low, lists_from_low(low, step=2)

    def chk0(m):
        assert m.item_head[:TILE].sum() == 256 and not m.item_head[TILE:].any()
    check(ctx, "256 heads in tile 0", h, loc, [False, True, False], model_check=chk0)


def test_constant_tile_without_a_head_continues_the_list_of_tile_0(ctx):
    n = 2 * TILE      # and the stream ends with the fast tile: its last element's id is the last list's last id
    h = np.full(n, H0 + 9)
    loc = np.cumsum(np.arange(n) % 5 + 1 + (np.arange(n) % 97 == 0) * 20000)

    def chk(m):
        assert len(m.hashes) == 1 and (m.item_len[TILE:] > 0).all() and set(m.item_len[TILE:]) == {1, 3} and int(m.last_ids[-1]) == loc[-1]
    check(ctx, "one list over a fast last tile", h, loc, [False, True], model_check=chk)


@pytest.mark.parametrize("kind", ["u16", "bucket"])
def test_offsets_join_across_general_and_fast_tiles(ctx, kind):
    n = 4 * TILE + 137      # tile 0 general, 1 fast, 2 with the change (general), 3 fast, 4 constant and partial (general)
    x = 2 * TILE + 700
    pre = np.where(np.arange(n) < x, B << 16 | U, (B << 16 | (U + 1)) if kind == "u16" else ((B + 1) << 16 | U))
    low = np.concatenate([np.arange(x) // 41, np.arange(n - x) // 53])      # lists start inside every tile and run across the tile ends
    assert low.max() < 256
    h = pre << 8 | low
    loc = lists_from_low(np.concatenate([[0], np.cumsum(h[1:] != h[:-1])]), step=77, rep=2)      # every second element a repeat

    def chk(m):
        for t in range(5):
            assert m.item_head[max(1, t * TILE):min(n, (t + 1) * TILE)].sum() > (8 if t < 4 else 1) and (m.item_len[t * TILE:(t + 1) * TILE] == 0).sum() > 0, t
        assert m.item_head[x] and (h[x] >> 8 != h[x - 1] >> 8)
    check(ctx, f"mixed paths, {kind} change", h, loc, [False, True, False, True, False], model_check=chk)


@pytest.mark.parametrize("shift", [0, 15])
@pytest.mark.parametrize("over", [0, 1], ids=["first_id + S = 2^28", "first_id + S = 2^28 + 1"])
def test_heads_up_to_and_across_2_28(ctx, over, shift):
    """the largest head of the call is 2^28 - 1 (four bytes, as every head), or one head is 2^28 (five bytes, and the two dwords one element can
    complete), in a fast tile behind alignment shifts 0 and 15"""
    S = 300
    first_id = (1 << 28) - S + over
    # tile 0: eight lists of 256 elements, ids 10, 11, ... then repeats of the last: a four-byte head and one-byte deltas; 8 * 203 = 8 mod 16 bytes
    # with 200 ids each, so the last list holds 8 (shift 0) or 7 (shift 15) more
    cnt = [200] * 7 + [200 + (8 if shift == 0 else 7)]
    low0 = np.arange(TILE) // 256
    loc0 = np.concatenate([np.minimum(np.arange(256), c - 1) + 10 for c in cnt])
    # tile 1 (fast): lists of 64 elements, ids 0, 4, 8, ..., 252; the last list is the single largest id, 299, then repeats of it
    low1 = 8 + np.arange(TILE) // 64
    loc1 = np.arange(TILE) % 64 * 4
    loc1[low1 == low1.max()] = S - 1
    low = np.concatenate([low0, low1, [low1.max() + 1] * 3])
    loc = np.concatenate([loc0, loc1, [1, 2, 2]])
    h = H0 + low
    assert low.max() < 256 and loc.max() == S - 1

    def chk(m):
        ids = m.item_delta[m.item_head]
        assert int(m.offsets[np.searchsorted(m.hashes, H0 + 8)]) % 16 == shift and m.item_head[TILE]
        assert int(ids.max()) == (1 << 28) - 1 + over and (m.item_len == 5).sum() == over and (m.item_len[m.item_head] >= 4).all()
        assert m.item_head[TILE:2 * TILE].sum() == 32
    check(ctx, f"heads at 2^28 over={over} shift={shift}", h, loc, [False, True, False], first_id=first_id, model_check=chk)
