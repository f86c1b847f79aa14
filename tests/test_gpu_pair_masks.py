"""The MSD index build's mask table (k_hash.hip: k_pair_count_msd<true> stores the pass masks of every (work item, partner), k_pair_emit2<..,
MASKS> replays them with fd_replay_block instead of running the distance filter again; fd_api_build.hip: WS_PAIR_MASKS).  Every case is built
with the default build (the table), once more with FDGPU_PAIR_MASKS=0 (the fallback: count without stores, emit with fd_filter_block) and
compared byte for byte — hashes, offsets, values — with each other and with oracle.build_index.  That the default build really took the table
is read from fdgpu_debug_last_build_mask_bytes: 8 bytes per column of the batch (the columns restated here), 0 for the fallback.

Structures are made like those of tests/test_gpu_emit_partner_fetch.py (its builders are used)."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import oracle
from tests import quantiser_edges as qe
from tests import test_gpu_emit_partner_fetch as pf

pytestmark = pytest.mark.gpu

ENV = ("FDGPU_DTAB", "FDGPU_EXACT", "FDGPU_MSD", "FDGPU_IDS32", "FDGPU_PAIR_MASKS")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def case_blobs():
    """every pair inside the cutoff: the triangular first block alone (2, 63, 64), a second tile (65), two full tiles (128), a third tile with an
    odd run tail (129) and an even one (130)"""
    r = _rng(21)
    return [(pf._blob(r, n), r.integers(0, 20, n)) for n in (2, 63, 64, 65, 128, 129, 130)]


def case_unhashable_tail():
    """100 residues whose last ten are unhashable: the permuted order ends in a dead run inside the second block"""
    r = _rng(22)
    aa = r.integers(0, 20, 100)
    aa[90:] = 255
    return [(pf._blob(r, 100, 9.0), aa)]


def case_empty_last_block():
    """128 hashable residues and five unhashable ones: in amino-acid order the third block of tile 0 (and the second of tile 1, the first of tile
    2) holds no hashable partner — the step that only carries `last`"""
    r = _rng(23)
    aa = r.integers(0, 20, 133)
    aa[r.choice(133, 5, replace=False)] = 255
    return [(pf._blob(r, 133, 9.0), aa)]


def case_all_unhashable():
    r = _rng(24)
    return [(pf._blob(r, 70), np.full(70, 255)), (pf._blob(r, 3), np.full(3, 255))]


def case_chain():
    """a 4,200-residue straight chain at 3.8 A spacing: 66 partner blocks for the first work item, most columns zero"""
    ca = np.zeros((4200, 3))
    ca[:, 0] = 3.8 * np.arange(4200)
    return [(ca, _rng(25).integers(0, 20, 4200))]


def case_together():
    """all of them with 300 two-residue structures in one batch, some of them in between: the columns of neighbouring work items abut"""
    r = _rng(26)
    small = [(pf._blob(r, 2, 3.0), r.integers(0, 20, 2)) for _ in range(300)]
    big = case_blobs() + case_unhashable_tail() + case_empty_last_block() + case_all_unhashable() + pf.case_one_lane_per_partner() + case_chain()
    out = small[:100]
    for k, s in enumerate(big):
        out += [s] + small[100 + 10 * k: 110 + 10 * k]
    return out + small[100 + 10 * len(big):]


CASES = {"blobs": case_blobs, "unhashable tail": case_unhashable_tail, "empty last block": case_empty_last_block, "all unhashable": case_all_unhashable,
         "one lane per partner": pf.case_one_lane_per_partner, "chain 4200": case_chain, "together": case_together}


def mask_columns(res_off):
    """columns of the batch's mask table (fd_pair_mask_cols.h): per 64-residue tile the partners up to the structure's end, in whole blocks"""
    n = 0
    for a, b in zip(res_off[:-1], res_off[1:]):
        R = int(b) - int(a)
        n += sum(-(-(R - t) // 64) * 64 for t in range(0, R, 64))
    return n


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    faulthandler.dump_traceback_later(600, exit=True)
    c = fd.Context(0)
    yield c
    c.close()
    faulthandler.cancel_dump_traceback_later()


_ORACLE = {}


def _oracle_of(name, d):
    if name not in _ORACLE:
        oix, _, _ = oracle.build_index(qe.to_oracle_structs(d))
        _ORACLE[name] = (oix.hashes().copy(), oix.offsets().copy(), oix.values().copy())
    return _ORACLE[name]


def _build(ctx, monkeypatch, packed, masks):
    """-> (values, hashes, offsets), bytes of the mask table the emit replayed, postings, fallbacks"""
    import folddisco_amd as fd
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if not masks:
        monkeypatch.setenv("FDGPU_PAIR_MASKS", "0")
    ctx.spec_fallbacks()
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(packed))
    mb = C.c_uint64(0)
    ctx.check(ctx.L.fdgpu_debug_last_build_mask_bytes(ctx.h, C.byref(mb)))
    monkeypatch.delenv("FDGPU_PAIR_MASKS", raising=False)
    return ix.export(), int(mb.value), ix.num_postings, ctx.spec_fallbacks()


def _same(a, b, what):
    for x, y, part in zip(a, b, ("values", "hashes", "offsets")):
        assert np.array_equal(x, y), (what, part)


def _check(ctx, monkeypatch, name, d, packed, ref):
    got, eb, np_on, _ = _build(ctx, monkeypatch, packed, True)
    off, eb0, np_off, _ = _build(ctx, monkeypatch, packed, False)
    cols = mask_columns(d["res_off"])
    print(f"{name}: {len(d['res_off']) - 1} structures, {cols} columns, {np_on} postings")
    assert (eb, eb0) == (8 * cols, 0) and np_on == np_off      # the default build read the table, the other did not
    _same(got, off, name + ": table vs filter")
    h, o, v = ref
    _same(got, (v, h, o), name + ": table vs oracle")
    _same(off, (v, h, o), name + ": filter vs oracle")


@pytest.mark.parametrize("name", list(CASES))
def test_table_build_equals_filter_build_and_oracle(ctx, monkeypatch, name):
    d = pf._layout(CASES[name]())
    _check(ctx, monkeypatch, name, d, qe.to_packed(d), _oracle_of(name, d))
    if name == "all unhashable":
        assert len(_oracle_of(name, d)[0]) == 0
    else:
        assert len(_oracle_of(name, d)[0]) > 0


def test_synthetic_database(ctx, monkeypatch):
    """synth.generate(2048, seed=1) both ways: the oracle's index, and the posting and fallback counts that
    test_gpu_emit_partner_fetch.test_synthetic_database records (33,431,018 pairs, 6,039 fallbacks)"""
    from folddisco_amd import synth
    from tests.helpers import packed_to_oracle_structs
    ps = synth.to_packed(synth.generate(2048, seed=1))
    oix, _, _ = oracle.build_index(packed_to_oracle_structs(ps))
    ref = (oix.values(), oix.hashes(), oix.offsets())
    cols = mask_columns(ps.res_off)
    for masks in (True, False):
        got, eb, n_post, n_fb = _build(ctx, monkeypatch, ps, masks)
        print(f"masks {masks}: pairs {n_post // 2}, fallbacks {n_fb}, mask bytes {eb}, columns {cols}")
        assert eb == (8 * cols if masks else 0)
        _same(got, ref, f"synth 2048, masks {masks}")
        assert (n_fb, n_post // 2) == (6039, 33431018)


def test_stale_table_of_another_build_does_not_matter(ctx, monkeypatch):
    """in one context: a large build with the table, a smaller one with the switch off, then the smaller one with the table directly behind it
    (the table then holds the large build's words wherever the count pass of this call does not write), then the large one again"""
    big, small = pf._layout(case_together()), pf._layout(case_empty_last_block() + case_unhashable_tail() + case_all_unhashable())
    ref_big, ref_small = _oracle_of("together", big), _oracle_of("stale small", small)
    for d, ref, masks in ((big, ref_big, True), (small, ref_small, False), (small, ref_small, True), (big, ref_big, True)):
        got, _, _, _ = _build(ctx, monkeypatch, qe.to_packed(d), masks)
        h, o, v = ref
        _same(got, (v, h, o), f"masks {masks}")
