"""The distance filter of the index build's pair kernels (fd_filter_block in csrc/k_hash.hip: k_pair_count_msd / k_pair_count2 / k_pair_emit2) on the
smallest shapes at which its loop can go wrong: partner blocks of 64 with an empty, odd or even partner count, the first block's `j > i` mask at
a tile edge, a last i-tile of one lane, runs of one residue type that are one partner long or cross a block, unhashable residues at the ends
of a block, and CA distances exactly on the cutoff and one ulp beyond it.

Every case is one batch of a handful of structures, built in the default form (amino-acid order, bucket-major stream) and with FDGPU_MSD=0
(chain order, structure-major stream) and compared byte for byte — hashes, offsets, value bytes, posting count — with oracle.build_index on
the same structures.  There is no tolerance and no case the oracle does not decide.

The NaN case: the oracle accepts a NaN CA coordinate in a hashable residue (its accept test is `!(d > cutoff)` like the device's), so the
case is kept: all pairs of that residue pass the filter on both sides."""
import faulthandler

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
FORMS = ({}, {"FDGPU_MSD": "0"})
LENGTHS = (1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 193)


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
    """a random walk of CA atoms (3.8 A steps: a 193-residue chain spans ~50 A, so pairs fall on both sides of every cutoff used here) with N and
    CB at their bond lengths in random directions -> dict(n, ca, cb, aa, ok)"""
    ca = np.cumsum(_unit(rng, n) * step, axis=0) + rng.uniform(-30.0, 30.0, size=3)
    aa = rng.integers(0, 20, size=n) if aa is None else np.asarray(aa)
    return dict(n=(ca + 1.46 * _unit(rng, n)).astype(np.float32), ca=ca.astype(np.float32), cb=(ca + 1.53 * _unit(rng, n)).astype(np.float32),
                aa=aa.astype(np.uint8), ok=np.ones(n, np.uint8))


def _layout(items):
    off = np.concatenate([[0], np.cumsum([len(s["aa"]) for s in items])]).astype(np.uint64)
    return dict(res_off=off, n_xyz=np.concatenate([s["n"] for s in items]), ca_xyz=np.concatenate([s["ca"] for s in items]),
                cb_xyz=np.concatenate([s["cb"] for s in items]), aa=np.concatenate([s["aa"] for s in items]),
                cb_ok=np.concatenate([s["ok"] for s in items]))


def _oracle_structs(items):
    return [oracle.structure_from_packed(s["n"], s["ca"], s["cb"], s["aa"], cb_ok=s["ok"]) for s in items]


def _postings(values):
    return len(values) - int(np.count_nonzero(values & 0x80))      # one terminator byte per posting


def _assert_forms_equal_oracle(ctx, monkeypatch, items, name, cutoff=20.0):
    """-> the oracle's index; both build forms equal it byte for byte"""
    import folddisco_amd as fd
    d = _layout(items)
    batch = ctx.upload(fd.PackedStructures(d["res_off"], d["n_xyz"], d["ca_xyz"], d["cb_xyz"], d["aa"], d["cb_ok"]))
    oix, _, _ = oracle.build_index(_oracle_structs(items), cutoff=cutoff)
    for form in FORMS:
        monkeypatch.delenv("FDGPU_MSD", raising=False)
        for k, v in form.items():
            monkeypatch.setenv(k, v)
        ix = fd.FolddiscoIndex.build(ctx, batch, dist_cutoff=cutoff)
        v, h, o = ix.export()
        print(f"{name} {form}: H={len(h)} bytes={len(v)} postings={ix.num_postings} (oracle H={oix.H} postings={_postings(oix.values())})")
        assert np.array_equal(h, oix.hashes()), (name, form)
        assert np.array_equal(o, oix.offsets()), (name, form)
        assert np.array_equal(v, oix.values()), (name, form)
        assert ix.num_postings == _postings(oix.values()), (name, form)
    monkeypatch.delenv("FDGPU_MSD", raising=False)
    return oix


def test_lengths_around_the_block_size(ctx, monkeypatch):
    """1 .. 193 residues: an empty partner loop (1), odd and even partner counts for the packed step, the first block's mask at the tile edge
    (63 / 64 / 65), a last i-tile of one lane (65, 129, 193) and of two (66)"""
    rng = np.random.default_rng(6401)
    oix = _assert_forms_equal_oracle(ctx, monkeypatch, [_chain(rng, n) for n in LENGTHS], "lengths")
    assert oix.H > 10000


def test_type_runs(ctx, monkeypatch):
    """one type over three blocks (a type below 16 and one above: both forward counters), a run boundary at nearly every partner with a run
    across the block edge (the 20 types in order, repeated to 65), only types >= 16, only types < 16"""
    rng = np.random.default_rng(6402)
    cyc = np.arange(65) % 20
    cyc[63:65] = 7                                   # one run across the edge of the first block (in chain order)
    items = [_chain(rng, 130, aa=np.full(130, 3)), _chain(rng, 130, aa=np.full(130, 18)), _chain(rng, 65, aa=np.arange(65) % 20), _chain(rng, 65, aa=cyc),
             _chain(rng, 97, aa=rng.integers(16, 20, size=97)), _chain(rng, 97, aa=rng.integers(0, 16, size=97))]
    oix = _assert_forms_equal_oracle(ctx, monkeypatch, items, "type runs")
    assert oix.H > 5000


def _unhashable(s, idx, how):
    for k, i in enumerate(idx):
        if (how == "cb") or (how == "mixed" and k % 2 == 0):
            s["ok"][i] = 0
        else:
            s["aa"][i] = 255
    return s


def test_unhashable_residues(ctx, monkeypatch):
    """missing CB / unknown type first, last, at 63 / 64 / 65, in every second position; none hashable; exactly one hashable.  In amino-acid
    order the hashable prefix then ends inside a block, at a block edge (128 residues, 64 hashable) and at zero"""
    rng = np.random.default_rng(6403)
    items = [_unhashable(_chain(rng, 130), [0], "cb"), _unhashable(_chain(rng, 130), [129], "aa"), _unhashable(_chain(rng, 130), [63, 64, 65], "mixed"),
             _unhashable(_chain(rng, 129), range(0, 129, 2), "mixed"), _unhashable(_chain(rng, 128), range(1, 128, 2), "cb"),
             _unhashable(_chain(rng, 70), range(70), "mixed"), _unhashable(_chain(rng, 70), [i for i in range(70) if i != 66], "aa"),
             _unhashable(_chain(rng, 66), [0, 65], "cb"), _unhashable(_chain(rng, 3), range(3), "cb"), _unhashable(_chain(rng, 1), [0], "aa")]
    oix = _assert_forms_equal_oracle(ctx, monkeypatch, items, "unhashable")
    assert oix.H > 5000


def _d2_max(cutoff):
    """largest f32 d2 with sqrt(d2) <= cutoff (float32 sqrt is correctly rounded): the constant the device compares with"""
    cut = np.float32(cutoff)
    d2 = np.float32(cut * cut)
    while np.sqrt(d2) > cut:
        d2 = np.nextafter(d2, np.float32(0))
    while np.sqrt(np.nextafter(d2, np.float32(np.inf))) <= cut:
        d2 = np.nextafter(d2, np.float32(np.inf))
    return d2


def _dist2_f32(a, b):
    """fd_dist2's operations in its order, every one rounded to float32"""
    dx, dy, dz = (a[..., 0] - b[..., 0]).astype(np.float32), (a[..., 1] - b[..., 1]).astype(np.float32), (a[..., 2] - b[..., 2]).astype(np.float32)
    return ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32) + (dz * dz).astype(np.float32)


def _pair_at(rng, target, tries=20000):
    """two float32 points whose squared distance, computed like fd_dist2, is exactly `target` -> (a, b) or None"""
    r = float(np.sqrt(np.float64(target)))
    a = rng.uniform(-40.0, 40.0, size=(tries, 3)).astype(np.float32)
    b = (a + (_unit(rng, tries) * r)).astype(np.float32)
    for _ in range(64):                               # walk b's x coordinate ulp by ulp towards the target
        d2 = _dist2_f32(a, b)
        hit = np.nonzero(d2 == target)[0]
        if len(hit):
            return a[hit[0]].copy(), b[hit[0]].copy()
        away = np.where(b[:, 0] >= a[:, 0], np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        b[:, 0] = np.where(d2 < target, np.nextafter(b[:, 0], away), np.nextafter(b[:, 0], -away))
    return None


def _three(rng, a, b):
    s = _chain(rng, 3)
    s["ca"][0], s["ca"][1], s["ca"][2] = a, b, a + np.float32(1000.0)
    u, v = _unit(rng, 3), _unit(rng, 3)
    s["n"], s["cb"] = (s["ca"] + 1.46 * u).astype(np.float32), (s["ca"] + 1.53 * v).astype(np.float32)
    return s


@pytest.mark.parametrize("cutoff", [20.0, 6.0, 25.0])
def test_cutoff_edge(ctx, monkeypatch, cutoff):
    """d2 == d2_max (accepted) and d2 == nextafter(d2_max, inf) (rejected), both asserted in numpy before anything is built"""
    rng = np.random.default_rng(6404 + int(cutoff))
    d2m = _d2_max(cutoff)
    above = np.nextafter(d2m, np.float32(np.inf))
    on, off = _pair_at(rng, d2m), _pair_at(rng, above)
    assert on is not None and off is not None, "the search found no pair on the cutoff"
    assert _dist2_f32(on[0], on[1]) == d2m and _dist2_f32(off[0], off[1]) == above and above > d2m
    assert np.sqrt(d2m) <= np.float32(cutoff) < np.sqrt(above)
    items = [_three(rng, *on), _three(rng, *off), _three(rng, on[1], on[0]), _three(rng, off[1], off[0]), _chain(rng, 70)]
    ostructs = _oracle_structs(items)
    assert [len(oracle.hash_structure(s, 0, 0, cutoff)) for s in ostructs[:4]] == [2, 0, 2, 0]      # the oracle draws the line where the device's constant does
    _assert_forms_equal_oracle(ctx, monkeypatch, items, f"cutoff {cutoff}", cutoff=cutoff)


def test_nan_coordinate_passes_the_filter(ctx, monkeypatch):
    """a NaN CA coordinate in a hashable residue: `!(d2 > d2_max)` is true, on the device as in the oracle"""
    rng = np.random.default_rng(6405)
    s = _chain(rng, 5)
    s["ca"][2, 1] = np.nan
    far = _chain(rng, 4, step=500.0)                  # no pair within the cutoff ...
    far["ca"][1, 0] = np.nan                          # ... but the NaN residue's
    assert len(oracle.hash_structure(_oracle_structs([far])[0])) == 6
    _assert_forms_equal_oracle(ctx, monkeypatch, [s, far, _chain(rng, 10)], "nan")


def test_first_block_mask_all_pairs_pass(ctx, monkeypatch):
    """64 residues on one CA position: every pair of the first (and only) block passes, so the mask `j > i` alone decides what is emitted —
    64 * 63 ordered pairs before dedup (the oracle's raw list, asserted), and the index of exactly those"""
    rng = np.random.default_rng(6406)
    s = _chain(rng, 64)
    s["ca"][:] = s["ca"][0]
    s["n"], s["cb"] = (s["ca"] + 1.46 * _unit(rng, 64)).astype(np.float32), (s["ca"] + 1.53 * _unit(rng, 64)).astype(np.float32)
    raw = oracle.hash_structure(_oracle_structs([s])[0])
    assert len(raw) == 64 * 63
    oix = _assert_forms_equal_oracle(ctx, monkeypatch, [s], "first block")
    assert oix.H == len(np.unique(raw)) and _postings(oix.values()) == oix.H
