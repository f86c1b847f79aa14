"""The digit planes of the MSD index build (csrc/k_hash.hip drain2 -> csrc/k_sort.hip fd_radix_sort_pairs16_seg -> the B24 codec of csrc/k_index.hip):
the 6-byte sort element is a u32 plane `hash[7:0] << 24 | local id` and a u16 plane `hash[23:8]`, the first sort pass takes its digit from the
u32 plane and the other two from the u16 plane, whose histogram reads eight elements per 16-byte load on full tiles.

Shapes chosen for where that split can go wrong: buckets that hold several full 8,192-key tiles between two cut ones next to an empty bucket, local
ids that cross 2^16 inside posting lists (the id no longer straddles the two planes) with a varint length boundary among the absolute ids, inputs
on which every one of the three digits and their order matter, and the smallest stream there is.

Every case is built in the default form and with FDGPU_MSD=0 and compared byte for byte — hashes, offsets, value bytes, posting count — with the
oracle's index of the same structures.  No tolerance.  The conditions a case is there for are asserted on the oracle's output before anything
is compared, so a case cannot silently stop covering them."""
import faulthandler

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
FORMS = ({}, {"FDGPU_MSD": "0"})
TILE = 8192                                           # keys per tile of the segmented sort (512 threads x 16)


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    faulthandler.dump_traceback_later(600, exit=True)
    c = fd.Context(0)
    yield c
    c.close()
    faulthandler.cancel_dump_traceback_later()


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _chain(rng, n, aa=None, step=3.8):
    """a random walk of CA atoms with N and CB at their bond lengths in random directions -> dict(n, ca, cb, aa, ok)"""
    ca = np.cumsum(_unit(rng, n) * step, axis=0) + rng.uniform(-30.0, 30.0, size=3)
    aa = rng.integers(0, 20, size=n) if aa is None else np.asarray(aa)
    return dict(n=(ca + 1.46 * _unit(rng, n)).astype(np.float32), ca=ca.astype(np.float32), cb=(ca + 1.53 * _unit(rng, n)).astype(np.float32),
                aa=aa.astype(np.uint8), ok=np.ones(n, np.uint8))


def _upload(ctx, items):
    import folddisco_amd as fd
    off = np.concatenate([[0], np.cumsum([len(s["aa"]) for s in items])]).astype(np.uint64)
    cat = lambda k: np.concatenate([s[k] for s in items])
    return ctx.upload(fd.PackedStructures(off, cat("n"), cat("ca"), cat("cb"), cat("aa"), cat("ok")))


def _oracle_struct(s):
    return oracle.structure_from_packed(s["n"], s["ca"], s["cb"], s["aa"], cb_ok=s["ok"])


def _list_postings(oix):
    """postings of every list of the oracle's index: one terminator byte (high bit clear) per posting"""
    term = np.concatenate([[0], np.cumsum((oix.values() & 0x80) == 0)])
    o = oix.offsets().astype(np.int64)
    return term[o[1:]] - term[o[:-1]]


def _assert_forms_equal(ctx, monkeypatch, batch, oix, name, first_id=0):
    import folddisco_amd as fd
    posts = int(_list_postings(oix).sum())
    for form in FORMS:
        monkeypatch.delenv("FDGPU_MSD", raising=False)
        for k, v in form.items():
            monkeypatch.setenv(k, v)
        ix = fd.FolddiscoIndex.build(ctx, batch, first_id=first_id)
        v, h, o = ix.export()
        print(f"{name} {form}: H={len(h)} bytes={len(v)} postings={ix.num_postings} (oracle H={oix.H} postings={posts})")
        assert np.array_equal(h, oix.hashes()), (name, form)
        assert np.array_equal(o, oix.offsets()), (name, form)
        assert np.array_equal(v, oix.values()), (name, form)
        assert ix.num_postings == posts, (name, form)
    monkeypatch.delenv("FDGPU_MSD", raising=False)


def test_full_tiles_between_cut_tiles_and_an_empty_bucket(ctx, monkeypatch):
    """36 chains of 200 residues of the types 3 and 18 only: four of the forty buckets (hash >> 24 = type_i << 1 | type_j >> 4: 6, 7, 36, 37) share all
    keys, so each holds a dozen 8,192-key tiles and the buckets between them none.  The u16 histogram takes its 16-byte path on the full tiles and
    its element-wise path on the two cut tiles of every bucket; the encoder's tiles cross the four boundaries."""
    rng = np.random.default_rng(7101)
    items = [_chain(rng, 200, aa=rng.choice([3, 18], size=200)) for _ in range(36)]
    structs = [_oracle_struct(s) for s in items]
    oix, _, _ = oracle.build_index(structs)
    per_bucket = np.bincount(oix.hashes() >> 24, weights=_list_postings(oix), minlength=64).astype(np.int64)
    # a bucket's keys are at least its postings, and a range of 3 * TILE keys or more holds two full aligned tiles wherever it starts
    assert per_bucket.max() >= 3 * TILE, per_bucket
    assert (per_bucket[:40] == 0).any() and per_bucket[40:].sum() == 0, per_bucket
    # where the buckets start in the key stream (keys = the raw pair lists, before the per-structure dedup): some bucket with two full tiles
    # or more starts and ends inside a tile
    raw = np.concatenate([oracle.hash_structure(s) for s in structs])
    assert int(raw.max()) < 1 << 30                   # the 6-byte element holds every hash: no rebuild with 8-byte elements
    start = np.concatenate([[0], np.cumsum(np.bincount(raw >> 24, minlength=40))])
    lo, hi = start[:-1], start[1:]
    full = hi // TILE - (lo + TILE - 1) // TILE
    assert ((full >= 2) & (lo % TILE != 0) & (hi % TILE != 0)).any(), (lo, hi)
    _assert_forms_equal(ctx, monkeypatch, _upload(ctx, items), oix, "tiles")


# ---- local ids across 2^16
N_MANY = (1 << 16) + 64
ODD_ONES = (0, 1, 39999, 40000, 65534, 65535, 65536, 65537, N_MANY - 1)      # structures with a geometry of their own: lists that START at these ids


@pytest.fixture(scope="module")
def many():
    """65,600 structures of three residues (two for the odd ones in every second place), all but nine of them one geometry -> (items, per-structure
    sorted-unique hash lists of the oracle as CSR, the oracle's index with ids from 0)"""
    rng = np.random.default_rng(7102)
    tmpl = _chain(rng, 3)
    odd = {s: _chain(rng, 2 + k % 2) for k, s in enumerate(ODD_ONES)}
    items = [odd.get(s, tmpl) for s in range(N_MANY)]
    o_tmpl = _oracle_struct(tmpl)
    o_odd = {s: _oracle_struct(v) for s, v in odd.items()}
    structs = [o_odd.get(s, o_tmpl) for s in range(N_MANY)]
    oix, _, _ = oracle.build_index(structs)
    h, off = oracle.hash_batch(structs)
    return items, h, off, oix


def test_local_ids_across_65536(ctx, monkeypatch, many):
    """posting lists of 65,591 consecutive ids: the local id runs through 65,535 -> 65,536 inside every one of them, and lists of one posting start
    on both sides of it"""
    items, h, off, oix = many
    posts = _list_postings(oix)
    assert posts.max() >= N_MANY - len(ODD_ONES) and (posts == 1).sum() >= len(ODD_ONES)
    for s in (65535, 65536):
        assert len(oix.entries(int(h[off[s]]))) == 1  # a list of its own that starts exactly there
    # the index over per-structure lists is the same index (the form the first_id case below needs)
    oix2 = oracle.build_index_from_lists(h, off)
    assert np.array_equal(oix2.hashes(), oix.hashes()) and np.array_equal(oix2.offsets(), oix.offsets()) and np.array_equal(oix2.values(), oix.values())
    _assert_forms_equal(ctx, monkeypatch, _upload(ctx, items), oix, "ids 2^16")


@pytest.mark.parametrize("first_id", [(1 << 21) - 40000, (1 << 21) - 65536])
def test_local_ids_across_65536_with_first_id(ctx, monkeypatch, many, first_id):
    """the same structures at ids first_id + s: list heads of three and of four varint bytes (2^21 lies at local id 40,000, then at 65,536 itself).
    The oracle's index: the same per-structure lists behind first_id empty structures"""
    items, h, off, _ = many
    oix = oracle.build_index_from_lists(h, np.concatenate([np.zeros(first_id, np.uint64), off]))
    heads = np.array([int(oix.entries(int(h[off[s]]))[0]) for s in ODD_ONES])
    assert np.array_equal(heads, first_id + np.array(ODD_ONES))
    assert (heads < 1 << 21).any() and (heads >= 1 << 21).any()
    _assert_forms_equal(ctx, monkeypatch, _upload(ctx, items), oix, f"ids 2^16 + {first_id}", first_id=first_id)


def test_all_three_digits_decide_the_order(ctx, monkeypatch):
    """six ordinary chains: every sorted byte of the hash takes many values, and hashes that agree in the two bytes of the u16 plane differ in the
    byte of the u32 plane — a pass that read its digit from the wrong plane or shift would leave the lists out of order"""
    rng = np.random.default_rng(7103)
    items = [_chain(rng, n) for n in (150, 97, 131, 64, 200, 77)]
    structs = [_oracle_struct(s) for s in items]
    oix, _, _ = oracle.build_index(structs)
    h = oix.hashes()
    assert int(h.max()) < 1 << 30
    d0, d1, d2 = h & 255, (h >> 8) & 255, (h >> 16) & 255
    assert min(len(np.unique(d)) for d in (d0, d1, d2)) >= 64
    hi = h >> 8                                        # bucket, d2, d1: the hashes are sorted, so equal ones are neighbours
    assert (hi[1:] == hi[:-1]).sum() >= 64
    _assert_forms_equal(ctx, monkeypatch, _upload(ctx, items), oix, "digits")


def test_one_residue_pair(ctx, monkeypatch):
    """one structure of two residues: two keys in two buckets or one, every tile partial, the encoder's predecessor logic at element 0"""
    rng = np.random.default_rng(7104)
    s = _chain(rng, 2, aa=[5, 17])
    oix, _, _ = oracle.build_index([_oracle_struct(s)])
    assert oix.H == 2 and _list_postings(oix).tolist() == [1, 1]
    _assert_forms_equal(ctx, monkeypatch, _upload(ctx, [s]), oix, "one pair")
