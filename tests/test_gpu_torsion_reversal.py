"""The torsion reversal set (tests/torsion_reversal_cases.py) through the C ABI on the GPU.  The index build decides each of the two dihedrals
of a residue pair once and uses the key for both torsion fields that read it (fd_geom.h, fd_pair_both_spec); on these pairs the reference's two
readings land in different bins, or sit a few ulps from doing so.  Raw lists and index bytes must equal the oracle's, every disagreeing pair must
have taken the exact routine, and on ordinary data the exact routine must stay as rare as it was."""
import faulthandler

import numpy as np
import pytest

import oracle
from tests import quantiser_edges as qe
from tests import torsion_reversal_cases as trc

pytestmark = pytest.mark.gpu

# Fallback share of the default build of synth.generate(2048, seed=1) at the commit before the dihedrals were decided once
# (profiles/torsion_once_bench_S542000.json, "spec_fallback_share"): the four-decision form with its 1/|X| margin.
PARENT_FALLBACK_SHARE = 8054 / 33431018          # 2.409e-4
MAX_SHARE_RATIO = 1.5


@pytest.fixture(scope="module")
def gpu():
    import folddisco_amd as fd
    faulthandler.dump_traceback_later(600, exit=True)
    ctx = fd.Context(0)
    yield ctx, trc.reversal_set()
    ctx.close()
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("layout", ["per pair", "packed"])
def test_lists_and_index_equal_oracle_and_disagreeing_pairs_fall_back(gpu, monkeypatch, layout):
    import folddisco_amd as fd
    ctx, rs = gpu
    for k in ("FDGPU_DTAB", "FDGPU_EXACT", "FDGPU_MSD"):
        monkeypatch.delenv(k, raising=False)
    d = rs.per_pair() if layout == "per pair" else rs.packed()
    batch = ctx.upload(qe.to_packed(d))
    h, off = fd.get_geometric_hash_as_u32(ctx, batch, sort_dedup=False)
    wh, woff = qe.oracle_lists(d, qe.DEFAULT)
    assert np.array_equal(off, woff)
    bad = np.nonzero(h != wh)[0]
    assert len(bad) == 0, (len(bad), int(bad[0]), hex(int(h[bad[0]])), hex(int(wh[bad[0]])))
    ctx.spec_fallbacks()
    v, hh, o = fd.FolddiscoIndex.build(ctx, batch).export()
    n_fb = ctx.spec_fallbacks()
    oix, _, _ = oracle.build_index(qe.to_oracle_structs(d))
    assert np.array_equal(hh, oix.hashes()) and np.array_equal(o, oix.offsets()) and np.array_equal(v, oix.values())
    n_bad = int(rs.disagree.any(1).sum())
    print(f"{layout}: fallbacks {n_fb} of {len(rs)} pairs, {n_bad} with readings that differ")
    # every disagreeing pair took the exact routine (the bytes above say so too); fewer fallbacks than pairs: decisions within 64 ulps of a
    # threshold were ACCEPTED and compared
    assert n_bad <= n_fb < len(rs)


def test_fallback_share_on_ordinary_data(gpu, monkeypatch):
    """the widened margin and the conditioning guards must not hand ordinary pairs to the out-of-line exact routine"""
    import folddisco_amd as fd
    from folddisco_amd import synth
    ctx, _ = gpu
    for k in ("FDGPU_DTAB", "FDGPU_EXACT", "FDGPU_MSD"):
        monkeypatch.delenv(k, raising=False)
    batch = ctx.upload(synth.to_packed(synth.generate(2048, seed=1)))
    ctx.spec_fallbacks()
    ix = fd.FolddiscoIndex.build(ctx, batch)
    n_fb = ctx.spec_fallbacks()
    share = n_fb / (ix.num_postings / 2)
    print(f"fallbacks {n_fb} of {ix.num_postings // 2} pairs: share {share:.4e}, parent {PARENT_FALLBACK_SHARE:.4e}")
    assert 0 < share <= MAX_SHARE_RATIO * PARENT_FALLBACK_SHARE
