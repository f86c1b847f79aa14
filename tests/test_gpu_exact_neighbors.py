"""Exact neighbours on the device (fdgpu_rowset_neighbors, Context.rowset_neighbors, indexio.row_neighbors, `neighbors --exact`): the device
form equals the host form and the plain statement byte for byte on the hand-made rows, for every first id, k, floor and split, from run to
run and for every counter budget; every reported overlap equals the pair intersect; the counter table is complete on a small database and
agrees with the count query; rows of one index against the lists of another; a built index pins the meaning against the batch hasher; the
refusals, wrong row lengths and a damaged list are errors that leave the context usable; the command against --host."""
import ctypes as C
import os

import numpy as np
import pytest

from folddisco_amd import indexio
from tests import exact_neighbor_cases as xc

pytestmark = pytest.mark.gpu

u32p = C.POINTER(C.c_uint32)
NO_ID = indexio.ROW_NO_ID


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hand_made(ctx):
    """the hand-made index resident at both first ids, its files, and the row set of the queries"""
    import folddisco_amd as fd
    out = {}
    for f in xc.FIRST_IDS:
        v, h, o = xc.index(f)
        ix = fd.FolddiscoIndex.load(ctx, h, o, v, xc.S, first_id=f)
        Q, taken = ix.rowset(f + xc.QUERIES, window=97)
        assert taken == len(xc.QUERIES)
        out[f] = (ix, (v, h, o, xc.S, f), Q)
    yield out
    for _, _, Q in out.values():
        Q.close()


# ---- 1. device == host == statement
@pytest.mark.parametrize("first_id", xc.FIRST_IDS)
def test_device_equals_host_and_statement(ctx, hand_made, first_id, monkeypatch):
    ix, files, Q = hand_made[first_id]
    ex = (first_id + xc.QUERIES).astype(np.uint32)
    for k in xc.KS:
        for T in xc.FLOORS:
            want = xc.statement(first_id, k, T)
            assert indexio.rows_neighbors_host(xc.rows_csr(xc.QUERIES), files, xc.LENGTHS, k=k, floor_e4=T, exclude=ex, threads=3).tobytes() == want.tobytes()
            for split in (1, 3, 64):
                monkeypatch.setenv("FDGPU_XN_SPLIT", str(split))
                got = ctx.rowset_neighbors(Q, ix, xc.LENGTHS, k=k, floor_e4=T, exclude=ex)
                assert got.dtype == indexio.ROW_NEIGHBOR_DTYPE and got.shape == want.shape and got.tobytes() == want.tobytes(), (k, T, split)
                assert ctx.rowset_neighbors(Q, ix, xc.LENGTHS, k=k, floor_e4=T, exclude=ex).tobytes() == got.tobytes(), (k, T, split)
    monkeypatch.delenv("FDGPU_XN_SPLIT")
    assert ctx.rowset_neighbors(Q, ix, xc.LENGTHS, k=8, floor=0.5, exclude=ex).tobytes() == xc.statement(first_id, 8, 5000).tobytes()
    assert ctx.rowset_neighbors(Q, ix, xc.LENGTHS, k=8).tobytes() == xc.statement(first_id, 8, 0, exclude_self=False).tobytes()


# ---- 2. counter budgets
@pytest.mark.parametrize("first_id", xc.FIRST_IDS)
def test_counter_budget_does_not_change_the_result(ctx, hand_made, first_id):
    ix, files, _ = hand_made[first_id]
    ks = np.arange(41, 48)                            # the twins: equal rows land in different blocks, so a counter left behind shows
    want = indexio.row_neighbors_from_rows(xc.rows_csr(ks), xc.rows_csr(), first_id, 32, 0, (first_id + ks).astype(np.uint32))
    Q, _ = ix.rowset(first_id + ks)
    ctx.enable_timing(True)
    with Q:
        for budget, blocks in ((4 * xc.S, 7), (4 * xc.S * 3, 3), (4 * xc.S * 4 - 1, 3), (4 * xc.S * 7, 1), (0, 1), (1, 7)):
            got = ctx.rowset_neighbors(Q, ix, xc.LENGTHS, k=32, exclude=(first_id + ks).astype(np.uint32), counter_bytes=budget)
            assert got.tobytes() == want.tobytes(), budget
            stages = [n for n, _, _ in ctx.last_timings()]
            assert stages.count("xn_count") == stages.count("xn_select") == blocks and stages[0] == "xn_upload" and stages[-1] == "xn_copy", (budget, stages)
    ctx.enable_timing(False)
    assert (want["flags"][2, :2] == 1).all() and want["inter"][2, 0] == xc.LENGTHS[43]
    # the driver: one result for every pool, window and budget
    ids = first_id + xc.QUERIES[::3]
    ex = ids.astype(np.uint32)
    host = indexio.row_neighbors_host(files, None, ids, xc.LENGTHS, k=8, floor_e4=1, exclude=ex, pool_hashes=5000, threads=2)
    for pool, window, budget in ((2, 16384, 0), (5000, 1, 4 * xc.S * 5), (1 << 40, 16, 4 * xc.S), (300, 16384, 0)):
        st = {}
        got = indexio.row_neighbors(ix, None, ids, xc.LENGTHS, k=8, floor_e4=1, exclude=ex, window=window, pool_hashes=pool, counter_bytes=budget, stats=st)
        assert got.tobytes() == host.tobytes() and (st["chunks"] == 1) == (pool == 1 << 40), (pool, window, budget)
    assert indexio.row_neighbors(ix, None, [], xc.LENGTHS, k=4).shape == (0, 4)


# ---- 3. the counters against the pair intersect, a complete small database, and the count query
def test_counts_equal_the_pair_intersect_and_the_count_query(ctx, hand_made):
    import folddisco_amd as fd
    inter_q = xc.intersections()
    ix, _, Q = hand_made[16200]
    got = ctx.rowset_neighbors(Q, ix, xc.LENGTHS, k=32)
    every, _ = ix.rowset(16200 + np.arange(xc.S), window=211)
    qs, rs = np.nonzero(got["id"] != NO_ID)
    with every:
        inter = ctx.rowset_intersect(Q, every, qs.astype(np.uint32), (got["id"][qs, rs] - 16200).astype(np.uint32))
    assert len(qs) > 3000 and np.array_equal(inter, got["inter"][qs, rs])
    assert np.array_equal(got["union"][qs, rs], xc.LENGTHS[xc.QUERIES][qs] + xc.LENGTHS[got["id"][qs, rs] - 16200] - inter)
    # 30 structures, k = 32: every structure that shares a hash is reported, so the records are the whole counter table
    v, h, o = xc.sub_index(30, 60, 900)
    sub = fd.FolddiscoIndex.load(ctx, h, o, v, 30, first_id=900)
    got = ctx.rowset_neighbors(Q, sub, xc.LENGTHS[30:60], k=32)
    for j in range(len(xc.QUERIES)):
        want = {900 + s: int(inter_q[j, 30 + s]) for s in range(30) if inter_q[j, 30 + s]}
        assert {int(r["id"]): int(r["inter"]) for r in got[j] if int(r["id"]) != NO_ID} == want, xc.QUERIES[j]
    # distinct query hashes: the count query's total_match_count is the same number
    pick = [xc.NAMES[n] for n in ("fam0_3", "twin43", "len65", "hub9", "len1000")]
    queries = [(np.array(xc.ROWS[q], np.uint32), np.zeros(len(xc.ROWS[q]), np.uint32), np.zeros(len(xc.ROWS[q]), np.uint32)) for q in pick]
    recs = fd.count_query_batch(ctx, ix, queries, np.ones(xc.S, np.float32))
    where = {int(k): j for j, k in enumerate(xc.QUERIES)}
    for q, r in zip(pick, recs):
        assert np.array_equal(r["total_match_count"], inter_q[where[q]][r["nid"] - 16200]) and len(r) == int((inter_q[where[q]] > 0).sum())


# ---- 4. rows of one index against the lists of another
def test_against_another_index(ctx, hand_made):
    import folddisco_amd as fd
    ix, files, Q = hand_made[16200]
    v, h, o = xc.against_index()
    n = len(xc.AGAINST_ROWS)
    ag = fd.FolddiscoIndex.load(ctx, h, o, v, n, first_id=xc.AGAINST_FIRST)
    ag_len = np.array([len(r) for r in xc.AGAINST_ROWS], np.uint32)
    QA, _ = ag.rowset(xc.AGAINST_FIRST + np.arange(n))
    with QA:
        for k, T in ((1, 0), (32, 0), (8, 5000)):
            want = indexio.row_neighbors_from_rows(xc.csr(xc.AGAINST_ROWS), xc.rows_csr(), 16200, k, T, None)
            assert ctx.rowset_neighbors(QA, ix, xc.LENGTHS, k=k, floor_e4=T).tobytes() == want.tobytes(), (k, T)
            back = indexio.row_neighbors_from_rows(xc.rows_csr(xc.QUERIES), xc.csr(xc.AGAINST_ROWS), xc.AGAINST_FIRST, k, T, None)
            assert ctx.rowset_neighbors(Q, ag, ag_len, k=k, floor_e4=T).tobytes() == back.tobytes(), (k, T)
        want = indexio.row_neighbors_from_rows(xc.csr(xc.AGAINST_ROWS), xc.rows_csr(), 16200, 32, 0, None)
        assert all((want[j]["id"] == NO_ID).all() for j in (1, 2, 3, 4, 7)) and want[5, 0]["flags"] == 1      # hashes below, above and in no list; a copy
        got = indexio.row_neighbors(ag, ix, xc.AGAINST_FIRST + np.arange(n), xc.LENGTHS, k=32, pool_hashes=300, window=7, counter_bytes=4 * xc.S * 2)
        assert got.tobytes() == want.tobytes()


# ---- 5. a built index pins the meaning
def test_built_index_equals_the_hasher(ctx):
    import folddisco_amd as fd
    from folddisco_amd import synth
    ps = synth.to_packed(synth.generate(180, seed=31))
    h, ho = fd.get_geometric_hash_as_u32(ctx, ctx.upload(ps), sort_dedup=True)
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(ps), first_id=7)
    d_len = np.diff(ho.astype(np.int64)).astype(np.uint32)
    assert np.array_equal(ix.signatures()["n"], d_len)
    pick = np.arange(20, 60)
    rows = lambda ks: (np.concatenate([h[int(ho[s]):int(ho[s + 1])] for s in ks]), np.concatenate([[0], np.cumsum(d_len[ks])]).astype(np.uint64))
    want = indexio.row_neighbors_from_rows(rows(pick), (h, ho), 7, 8, 0, (7 + pick).astype(np.uint32))
    got = indexio.row_neighbors(ix, None, 7 + pick, d_len, k=8, exclude=(7 + pick).astype(np.uint32), window=16, pool_hashes=60000)
    assert got.tobytes() == want.tobytes() and (want["id"] != NO_ID).any() and want["inter"].max() > 1


# ---- 6. refusals and errors
def test_refusals_and_errors_leave_the_context_usable(ctx, hand_made):
    import folddisco_amd as fd
    ix, _, Q = hand_made[16200]
    L = ctx.L
    ex = (16200 + xc.QUERIES).astype(np.uint32)
    want = xc.statement(16200, 8, 0)
    ctx.enable_timing(True)
    assert ctx.rowset_neighbors(Q, ix, xc.LENGTHS, k=8, exclude=ex).tobytes() == want.tobytes()
    before = [n for n, _, _ in ctx.last_timings()]
    assert before[0] == "xn_upload" and "xn_count" in before and "xn_select" in before and before[-1] == "xn_copy"

    def call(Qh=Q.h, Dh=ix.h, d_len=xc.LENGTHS, exclude=None, k=8, T=0):
        out = C.c_void_p(1)
        arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.uint32).ctypes.data_as(u32p)
        rc = L.fdgpu_rowset_neighbors(ctx.h, Qh, Dh, arr(d_len), arr(exclude), k, T, 0, C.byref(out))
        return rc, out.value, L.fdgpu_last_error(ctx.h).decode()
    for kw in (dict(k=0), dict(k=33), dict(T=10001), dict(d_len=None), dict(Qh=None), dict(Dh=None), dict(exclude=np.where(ex == ex[5], 16199, ex)),
               dict(exclude=np.where(ex == ex[-1], 16200 + xc.S, ex)), dict(exclude=np.where(ex == ex[0], 0, ex))):
        rc, out, msg = call(**kw)
        assert (rc, out) == (-1, None) and msg.startswith("rowset neighbors:"), (kw, msg)
        assert [n for n, _, _ in ctx.last_timings()] == before
    ctx.enable_timing(False)
    assert L.fdgpu_rowset_neighbors(ctx.h, Q.h, ix.h, xc.LENGTHS.ctypes.data_as(u32p), None, 8, 0, 0, None) == -1
    # row lengths that are not the index's: one entry lowered, and a twin of that structure asks
    low = xc.LENGTHS.copy()
    low[44] -= 1
    with pytest.raises(fd.FdgpuError, match="row lengths do not belong to this index"):
        ctx.rowset_neighbors(Q, ix, low, k=8, exclude=ex)
    assert ctx.rowset_neighbors(Q, ix, xc.LENGTHS, k=8, exclude=ex).tobytes() == want.tobytes()
    # a damaged list is an error: the id at first_id + S is refused by the range test that stands before every counter address
    v, h, o = xc.damaged_index(16200)
    bad = fd.FolddiscoIndex.load(ctx, h, o, v, xc.S, first_id=16200)
    rc, out, msg = call(Dh=bad.h, exclude=ex)
    assert (rc, out) == (-1, None) and msg.startswith("rowset neighbors: the index is damaged"), msg
    assert ctx.rowset_neighbors(Q, ix, xc.LENGTHS, k=8, exclude=ex).tobytes() == want.tobytes()
    # empty sets and empty rows
    E, _ = ix.rowset([])
    assert ctx.rowset_neighbors(E, ix, xc.LENGTHS, k=5).shape == (0, 5)
    Z, _ = ix.rowset([16200, 16200 + 300])
    assert (ctx.rowset_neighbors(Z, ix, xc.LENGTHS, k=5)["id"] == NO_ID).all()
    E.close(), Z.close()


# ---- 7. the command
def test_neighbors_exact_command_equals_host(tmp_path, capsys):
    one, two, dev, host, tf = (str(tmp_path / n) for n in ("one", "two", "dev.tsv", "host.tsv", "tids.txt"))
    tids = xc.write_index(one)
    xc.write_index(two, rows=xc.AGAINST_ROWS, tids=[f"u{k}" for k in range(40)])
    with open(tf, "w") as f:
        f.writelines(f"{tids[k]}\n" for k in xc.QUERIES[::2])
    capsys.readouterr()
    for extra in (["-i", one, "--verify", "--window", "50", "--counter-mb", "1"], ["-i", one, "--tids", tf, "-k", "32", "--min-jaccard", "0.02"],
                  ["-i", two, "--against", one, "-k", "3"], ["-i", one, "--against", two, "--tids", tf, "--min-jaccard", "0.5"]):
        assert xc.status(["neighbors", "--exact", "-o", dev, "-v"] + extra) == 0
        cap = capsys.readouterr()
        assert xc.status(["neighbors", "--exact", "--host", "-o", host] + extra) == 0
        assert capsys.readouterr().out == cap.out and "[INFO] neighbors --exact on the device" in cap.err
        assert open(dev).read() == open(host).read() and ", exact, " in cap.out
        assert extra[1] != one or open(dev).read().count("\n") > 0
    names = sorted(os.listdir(tmp_path))
    assert xc.status(["neighbors", "-i", one, "-o", dev, "--min-jaccard", "0.5"]) == 1
    assert xc.status(["neighbors", "--exact", "-i", one, "-o", dev, "--confirm"]) == 1
    assert xc.status(["neighbors", "--exact", "-i", one, "-o", dev, "--min-similarity", "0.5"]) == 1
    assert sorted(os.listdir(tmp_path)) == names
