"""The pair scan's output regrow (mp_scan, csrc/fd_api_match.hip): a scan whose found triples do not fit the first allocation of a fresh context
(65,536 records) only counts, the buffers grow and the scan is launched once more; the next identical call fits at once.

One query of 640 hashes (every 24th residue pair inside the cutoff of a 200-residue structure, window 0.01 A) against 104 candidate slots that all
name that structure: the numpy model of retrieval_cases.py gives 642 found triples and 736 candidate pairs per slot, 66,768 and 76,544 in all.  The
pairs are spread over the structure so that no work item queues more than a few chunks: the chunk queue must not regrow as well (a third launch)."""
import numpy as np
import pytest

from tests import retrieval_cases as rc

pytestmark = pytest.mark.gpu

COPIES, FOUND_PER_SLOT, CANDS_PER_SLOT, WINDOW = 104, 642, 736, 0.01
FIRST_CAPACITY = 65536


def test_output_regrow_repeats_the_scan_once():
    import folddisco_amd as fd
    from folddisco_amd import match
    T = rc.base(200)
    b = rc.MapBuilder(T)
    ii, jj = np.nonzero(T.valid)
    for i, j in list(zip(ii.tolist(), jj.tolist()))[::len(ii) // 640][:640]:
        b.edge(i, j)
    a = b.arrays([0, 1])
    want_found, want_cand = rc.model_scan(T, a, WINDOW)
    assert (len(want_found), len(want_cand)) == (FOUND_PER_SLOT, CANDS_PER_SLOT) and COPIES * FOUND_PER_SLOT > FIRST_CAPACITY
    ctx = fd.Context(0)          # fresh: no output buffer yet
    try:
        db = ctx.upload(fd.PackedStructures.concat([T.item]))
        ctx.enable_timing(True)
        runs = []
        for launches in (2, 1):
            found, cands = match.match_pairs(ctx, db, None, np.zeros(COPIES, np.uint32), rc.match_query(a), ca_distance_cutoff=WINDOW)
            ctx.synchronize()
            assert [n for n, _, _ in ctx.last_timings()] == ["match_pairs"] * launches
            runs.append((found, cands))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        found, cands = runs[0]
        assert len(found) == COPIES * FOUND_PER_SLOT and len(cands) == COPIES * CANDS_PER_SLOT
        for k in (0, COPIES - 1):
            assert np.array_equal(found[found[:, 0] == k][:, 1:].astype(np.uint64), want_found) and np.array_equal(cands[cands[:, 0] == k][:, 1:].astype(np.uint64), want_cand)
    finally:
        ctx.close()
