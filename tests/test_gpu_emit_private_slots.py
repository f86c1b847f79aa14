"""The MSD index build's slot tables (k_hash.hip: k_pair_count_msd, k_pair_emit2<.., MSD>; fd_api_build.hip: ib_count_msd, ib_emit_msd).  The count pass
writes counts[bucket][work item] for all forty buckets of every work item (a work item = one 64-residue tile of a structure in amino-acid
order), zeros included and without clearing the table first; the exclusive scan of the table gives every work item private, contiguous slots
in every bucket, and the emit pass fills them from a cursor in LDS.  The frames are built by the count work item that owns the tile, through
the source index of k_frames_perm's stable sort by residue type.

The cases are hand-made in the way of tests/test_gpu_emit_partner_fetch.py (blobs inside the cutoff, lattices beyond it): tiles of 1, 63, 64
and 65 lanes; work items that own nothing in the middle of the table; buckets that stay empty at either end of the forty; a batch without
any pair; builds of different shape one after the other on one context (nothing of a previous call's tables may show); the same batch twice.
Every build is compared byte for byte with oracle.build_index, some also with the structure-major build (FDGPU_MSD=0).

test_count_table_restated needs no GPU: it restates what the count pass must write per (bucket, work item) and checks it against the
oracle's hashes."""
import faulthandler

import numpy as np
import pytest

import oracle
from tests import quantiser_edges as qe

D2_MAX = np.float32(400.0)      # largest f32 whose square root is <= 20
TILE = 64
BUCKETS = 40


# ---- structures ------------------------------------------------------------------------------------------------------------------------------
def _residues(rng, ca):
    """N, CA, CB of residues at the given CA positions, side chains in random directions (the construction of quantiser_edges._draw)"""
    ca = np.asarray(ca, np.float64)
    n = len(ca)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    w = rng.normal(size=(n, 3))
    w -= (w * u).sum(1)[:, None] * u
    w /= np.linalg.norm(w, axis=1)[:, None]
    cb = ca + rng.uniform(qe.BOND_MIN, qe.BOND_MAX, n)[:, None] * u
    nn = ca + 1.46 * (-0.33 * u + 0.94 * w)
    return nn.astype(np.float32), ca.astype(np.float32), cb.astype(np.float32)


def _layout(structs):
    """[(ca positions, aa)] -> the layout dict of quantiser_edges (to_packed / to_oracle_structs)"""
    rng = np.random.Generator(np.random.PCG64(707))
    N, CA, CB, AA, off = [], [], [], [], [0]
    for ca, aa in structs:
        n, c, b = _residues(rng, ca)
        N.append(n); CA.append(c); CB.append(b); AA.append(np.asarray(aa, np.uint8))
        off.append(off[-1] + len(aa))
    return dict(res_off=np.asarray(off, np.uint64), n_xyz=np.concatenate(N), ca_xyz=np.concatenate(CA), cb_xyz=np.concatenate(CB), aa=np.concatenate(AA))


def _blob(rng, n, radius=9.0):
    """n CA positions inside a ball: every pair is closer than 2 * radius < 20 A"""
    p = rng.normal(size=(n, 3))
    p *= (radius * rng.uniform(0.2, 1.0, n) ** (1 / 3) / np.linalg.norm(p, axis=1))[:, None]
    return p


def _lattice(n, step=100.0):
    g = np.arange(5) * step
    return np.array([[x, y, z] for x in g for y in g for z in g], np.float64)[:n]


BOUNDARY_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 200)


def case_tile_boundaries():
    """structures that end one residue short of, on and one residue past a tile edge, all pairs inside the cutoff, random types"""
    rng = np.random.Generator(np.random.PCG64(21))
    return [(_blob(rng, n), rng.integers(0, 20, n)) for n in BOUNDARY_SIZES]


def case_owns_nothing():
    """between two ordinary structures: one whose residues are all unhashable and one whose residues are 100 A apart — two work items each
    that own no slot in any bucket (zero-length segments in the middle of every bucket's table), and frames of unhashable residues"""
    rng = np.random.Generator(np.random.PCG64(22))
    return [(_blob(rng, 70), rng.integers(0, 20, 70)), (_blob(rng, 70), [255] * 70), (_lattice(70), rng.integers(0, 20, 70)),
            (_blob(rng, 90), rng.integers(0, 20, 90))]


def _typed(seed, lo, hi):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [(_blob(rng, n), rng.integers(lo, hi, n)) for n in (65, 10, 130)]


def case_low_types():
    """types 0-3 only: buckets 0-7 hold every key, 8-39 none"""
    return _typed(23, 0, 4)


def case_high_types():
    """types 16-19 only: buckets 33, 35, 37 and 39 hold every key, 0-32 none"""
    return _typed(24, 16, 20)


def case_one_type():
    """one type in the whole batch: one bucket"""
    return _typed(25, 7, 8)


CASES = {"tile boundaries": case_tile_boundaries, "owns nothing": case_owns_nothing, "low types": case_low_types, "high types": case_high_types,
         "one type": case_one_type}


# ---- the count pass, restated ------------------------------------------------------------------------------------------------------------------
def count_table(structs):
    """counts[bucket][work item] as k_pair_count_msd must write them, and the structure of every work item.  A structure's residues are
    sorted stably by type (unhashable ones last) and cut into tiles of 64; a work item counts the pairs (i in its tile, j behind i in that
    order, both hashable, squared CA distance not above 400 in f32) in both orientations: bucket type_i * 2 + (type_j >> 4) and
    type_j * 2 + (type_i >> 4)"""
    cols, owner = [], []
    for s, (ca, aa) in enumerate(structs):
        aa = np.asarray(aa).astype(np.int64)
        ok = aa < 20
        order = np.argsort(np.where(ok, aa, 20), kind="stable")
        ca = np.asarray(ca, np.float64).astype(np.float32)[order]
        t, ok = aa[order], ok[order]
        n = len(t)
        d = ca[:, None, :] - ca[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]      # f32, fd_dist2's order
        passes = ~(d2 > D2_MAX) & ok[:, None] & ok[None, :] & (np.arange(n)[:, None] < np.arange(n)[None, :])
        for i0 in range(0, n, TILE):
            col = np.zeros(BUCKETS, np.int64)
            i, j = np.nonzero(passes[i0:i0 + TILE])
            i += i0
            np.add.at(col, t[i] * 2 + (t[j] >> 4), 1)
            np.add.at(col, t[j] * 2 + (t[i] >> 4), 1)
            cols.append(col)
            owner.append(s)
    return np.array(cols, np.int64).reshape(-1, BUCKETS).T, np.array(owner, np.int64)


def _list_postings(oix):
    """postings of the oracle's index: one terminator byte (high bit clear) per posting"""
    return int(np.count_nonzero((oix.values() & 0x80) == 0))


def test_count_table_restated():
    """no GPU: the restated table of the tile-boundary batch against the oracle.  Per structure and bucket, the work items' counts sum to the
    number of the structure's hashes with those top six bits; the table's sum is the oracle's key count, and less the keys that repeat a hash
    inside their structure (the index keeps one posting per hash and structure) the posting count of oracle.build_index"""
    structs = case_tile_boundaries()
    d = _layout(structs)
    # the layout rounds the CA positions to f32 once; the restatement reads the same f32 values
    off = d["res_off"].astype(np.int64)
    table, owner = count_table([(d["ca_xyz"][off[s]:off[s + 1]], aa) for s, (_, aa) in enumerate(structs)])
    assert table.shape == (BUCKETS, sum((n + TILE - 1) // TILE for n in BOUNDARY_SIZES)) and table.shape[1] == 17
    ostructs = qe.to_oracle_structs(d)
    repeats = 0
    total = np.zeros(BUCKETS, np.int64)
    for s, os_ in enumerate(ostructs):
        h = oracle.hash_structure(os_)
        per_bucket = np.bincount(h >> 24, minlength=BUCKETS)
        assert len(per_bucket) == BUCKETS
        assert np.array_equal(table[:, owner == s].sum(1), per_bucket), s
        repeats += len(h) - len(np.unique(h))
        total += per_bucket
    assert np.array_equal(table.sum(1), total)
    oix, _, _ = oracle.build_index(ostructs)
    assert table.sum() - repeats == _list_postings(oix)
    assert table[:, owner == 0].sum() == 0 and table[:, owner == 1].sum() == 2      # one residue: no pair; two residues: one pair, two keys
    assert table.sum() == sum(n * (n - 1) for n in BOUNDARY_SIZES)                   # every pair passes


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def ctx():
    import folddisco_amd as fd
    faulthandler.dump_traceback_later(600, exit=True)
    c = fd.Context(0)
    yield c
    c.close()
    faulthandler.cancel_dump_traceback_later()


def _default_env(monkeypatch):
    for k in ("FDGPU_DTAB", "FDGPU_EXACT", "FDGPU_MSD", "FDGPU_IDS32"):
        monkeypatch.delenv(k, raising=False)


def _assert_same(got, want, what):
    for a, b, name in zip(got, want, ("values", "hashes", "offsets")):
        assert np.array_equal(a, b), (what, name)


def _assert_index(got, oix, what):
    _assert_same(got, (oix.values(), oix.hashes(), oix.offsets()), what)


def _build(ctx, monkeypatch, packed, msd=True, first_id=0):
    import folddisco_amd as fd
    _default_env(monkeypatch)
    if not msd:
        monkeypatch.setenv("FDGPU_MSD", "0")
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(packed), first_id=first_id)
    monkeypatch.delenv("FDGPU_MSD", raising=False)
    return ix


@pytest.fixture(scope="module")
def synth_a():
    """about 300 structures of the generator and their oracle index, computed once"""
    from folddisco_amd import synth
    from tests.helpers import packed_to_oracle_structs
    ps = synth.to_packed(synth.generate(300, seed=5))
    return ps, oracle.build_index(packed_to_oracle_structs(ps))[0]


@pytest.fixture(scope="module")
def boundaries():
    d = _layout(case_tile_boundaries())
    return d, oracle.build_index(qe.to_oracle_structs(d))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in CASES if k != "tile boundaries"])
def test_hand_made_case_equals_oracle(ctx, monkeypatch, name):
    d = _layout(CASES[name]())
    oix, _, _ = oracle.build_index(qe.to_oracle_structs(d))
    assert oix.H > 0
    _assert_index(_build(ctx, monkeypatch, qe.to_packed(d)).export(), oix, name)


@pytest.mark.gpu
def test_tile_boundaries(ctx, monkeypatch, boundaries):
    d, oix = boundaries
    assert oix.H > 0
    got = _build(ctx, monkeypatch, qe.to_packed(d)).export()
    _assert_index(got, oix, "tile boundaries")
    _assert_same(got, _build(ctx, monkeypatch, qe.to_packed(d), msd=False).export(), "tile boundaries, structure-major")


@pytest.mark.gpu
def test_tile_boundaries_first_id(ctx, monkeypatch, boundaries):
    """the same batch as structures 1000 .. 1008.  The oracle's index: the same per-structure hash lists behind 1000 empty structures"""
    d, oix0 = boundaries
    lists = [np.unique(oracle.hash_structure(s)) for s in qe.to_oracle_structs(d)]      # sorted, one entry per hash: what the oracle's builder takes
    off = np.concatenate([[0], np.cumsum([len(h) for h in lists])]).astype(np.uint64)
    assert np.array_equal(oracle.build_index_from_lists(np.concatenate(lists), off).values(), oix0.values())      # the lists ARE the index's
    oix = oracle.build_index_from_lists(np.concatenate(lists), np.concatenate([np.zeros(1000, np.uint64), off]))
    assert int(oix.entries(int(oix.hashes()[0]))[0]) >= 1000
    got = _build(ctx, monkeypatch, qe.to_packed(d), first_id=1000).export()
    _assert_index(got, oix, "first_id 1000")
    _assert_same(got, _build(ctx, monkeypatch, qe.to_packed(d), msd=False, first_id=1000).export(), "first_id 1000, structure-major")


@pytest.mark.gpu
def test_one_residue_alone(ctx, monkeypatch):
    """one structure of one residue: one work item, no pair, every count zero.  As before the tables were per work item (read from
    index_build_impl: P = 0, the sort returns at once, the encoder makes an index of no list) the build gives an empty index, no error"""
    rng = np.random.Generator(np.random.PCG64(26))
    d = _layout([(_blob(rng, 1), [5])])
    oix, _, _ = oracle.build_index(qe.to_oracle_structs(d))
    assert oix.H == 0
    for msd in (True, False):
        ix = _build(ctx, monkeypatch, qe.to_packed(d), msd=msd)
        v, h, o = ix.export()
        assert ix.num_hashes == 0 and ix.num_postings == 0 and ix.value_len == 0
        assert len(v) == 0 and len(h) == 0 and o.tolist() == [0]


@pytest.mark.gpu
def test_stale_tables(ctx, monkeypatch, synth_a, boundaries):
    """a large batch, a small one, the large one again on ONE context: the tables are not cleared between calls and are written in full by
    every call, so each index equals its oracle's"""
    ps, oix_a = synth_a
    d, oix_b = boundaries
    _assert_index(_build(ctx, monkeypatch, ps).export(), oix_a, "first build")
    _assert_index(_build(ctx, monkeypatch, qe.to_packed(d)).export(), oix_b, "small build after a large one")
    _assert_index(_build(ctx, monkeypatch, ps).export(), oix_a, "large build after a small one")


@pytest.mark.gpu
def test_same_stream_twice(ctx, monkeypatch):
    from folddisco_amd import synth
    from tests.helpers import packed_to_oracle_structs
    ps = synth.to_packed(synth.generate(256, seed=3))
    oix, _, _ = oracle.build_index(packed_to_oracle_structs(ps))
    first = _build(ctx, monkeypatch, ps).export()
    second = _build(ctx, monkeypatch, ps).export()
    _assert_same(first, second, "second build")
    _assert_index(first, oix, "synth 256")
    _assert_same(first, _build(ctx, monkeypatch, ps, msd=False).export(), "structure-major")
