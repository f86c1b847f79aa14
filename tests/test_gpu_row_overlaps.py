"""Exact row overlaps on the device (fdgpu_index_rowset, fdgpu_rowset_intersect, FolddiscoIndex.rowset, Context.rowset_intersect,
indexio.row_overlaps, `python -m folddisco_amd overlap`): a row set's export equals the selected rows of the index and follows the budget rule;
the intersect equals the host form, the numpy statement and Python sets on every pair of the hand-made rows; the tiling driver gives one
result for every pool and window; a built index pins the meaning against the batch hasher; the refusals; the commands against --host."""
import ctypes as C
import os

import numpy as np
import pytest

from folddisco_amd import indexio
from tests import overlap_cases as oc
from tests.test_row_overlaps_host import POOLS, WINDOWS, _reaches, _status, write_index

pytestmark = pytest.mark.gpu

u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def every():
    ka, kb = oc.all_pairs()
    return ka, kb, oc.expected(ka, kb)


@pytest.fixture(scope="module")
def hand_made(ctx):
    """the hand-made index resident at both first ids, with its source arrays"""
    import folddisco_amd as fd
    out = {}
    for f in oc.FIRST_IDS:
        v, h, o = oc.index(f)
        out[f] = (fd.FolddiscoIndex.load(ctx, h, o, v, oc.N, first_id=f), (v, h, o))
    return out


def _eq(a, b):
    return len(a) == len(b) == 2 and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def _taken(lens, max_hashes):
    """the budget rule of the header: the largest t with t <= 1 or lens[0] + .. + lens[t - 1] <= max_hashes (0: no limit)"""
    t, total = 0, 0
    for L in lens:
        if max_hashes and t > 0 and total + L > max_hashes:
            break
        total += L
        t += 1
    return t


# ---- 1. export against rows
@pytest.mark.parametrize("first_id", oc.FIRST_IDS)
def test_rowset_export_equals_the_rows(ctx, hand_made, first_id):
    ix, src = hand_made[first_id]
    rows = ix.rows()
    assert _eq(rows, oc.rows_csr())                                               # the index holds the prescribed rows
    k_all = np.arange(oc.N)
    empties = [oc.NAMES["len0"], oc.NAMES["copy0"]]
    for ks in (k_all, k_all[:0], k_all[37:38], k_all[::2], np.array(empties), np.array(sorted(empties + [oc.NAMES["len4200"], oc.N - 1]))):
        for window in (1, 2, 7, 16384):
            rs, n_taken = ix.rowset(first_id + ks, window=window)
            with rs:
                want = oc.rows_csr(ks)
                assert n_taken == len(ks) == rs.n_rows and rs.n_hashes == len(want[0])
                assert _eq(rs.export(), want), (ks[:3], window)
                assert np.array_equal(rs.lengths(), np.diff(want[1].astype(np.int64)).astype(np.uint32)) and rs.lengths().dtype == np.uint32
            assert rs.h is None
    # the budget: the first row is always taken, the set stops before the row that would bring it above the limit, whatever the window
    for start in (0, oc.NAMES["len4200"], oc.NAMES["len1000"]):
        ks = k_all[start:]
        lens = [len(oc.ROWS[k]) for k in ks]
        for max_hashes in (1, 64, 4199, 4200, 4201, 0):
            t = _taken(lens, max_hashes)
            for window in (1, 7, 16384):
                rs, n_taken = ix.rowset(first_id + ks, window=window, max_hashes=max_hashes)
                assert n_taken == t == rs.n_rows and _eq(rs.export(), oc.rows_csr(ks[:t])), (start, max_hashes, window)
                rs.close()
    assert _taken([4200, 4200], 1) == 1 and _taken([0, 0, 1, 1, 2], 1) == 3 and _taken([4200, 0, 5], 4200) == 2 and _taken([3, 4], 0) == 2
    a, _ = ix.rowset(first_id + k_all[::3], window=5)                             # two runs give the same bytes
    b, _ = ix.rowset(first_id + k_all[::3], window=5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.export(), b.export()))
    a.close(), b.close()
    assert all(np.array_equal(x, y) for x, y in zip(ix.export(), src))            # the index is not changed


# ---- 2. intersect
def test_intersect_equals_host_numpy_and_python(ctx, hand_made, every):
    ix, _ = hand_made[5]
    ka, kb, want = every
    A, _ = ix.rowset(5 + np.arange(oc.N), window=9)
    rows = A.export()
    got = ctx.rowset_intersect(A, None, ka, kb)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(ctx.rowset_intersect(A, A, ka, kb), want)
    for threads in (1, 3):
        assert np.array_equal(indexio.rows_intersect_host(rows, None, ka, kb, threads=threads), got)
    assert np.array_equal(indexio.row_overlaps_from_rows(rows, None, ka, kb), got)
    na, nb, nw = oc.named_pairs()
    assert np.array_equal(ctx.rowset_intersect(A, None, na, nb), nw)
    # A against B: another set, of another index object, whose slots are not A's
    pick = np.array(sorted(oc.NAMES[n] for n in ("third", "len0", "top", "edge_q", "edge_q1", "len4200", "odds", "zero", "copy64", "ends_b")))
    B, _ = hand_made[0][0].rowset(pick, window=4)
    sa, sb = np.repeat(np.arange(oc.N, dtype=np.uint32), len(pick)), np.tile(np.arange(len(pick), dtype=np.uint32), oc.N)
    want_b = oc.expected(sa, pick[sb])
    assert np.array_equal(ctx.rowset_intersect(A, B, sa, sb), want_b)
    assert np.array_equal(ctx.rowset_intersect(B, A, sb, sa), want_b)
    assert np.array_equal(indexio.rows_intersect_host(rows, B.export(), sa, sb, threads=3), want_b)
    # the result is in input order: by work descending, ascending, the same pair twice; and the same bytes from run to run
    w = oc.work(ka, kb)
    for order in (np.argsort(-w, kind="stable"), np.argsort(w, kind="stable"), np.array([5, 5, 70, 5, 70])):
        assert np.array_equal(ctx.rowset_intersect(A, None, ka[order], kb[order]), want[order])
    assert ctx.rowset_intersect(A, None, ka, kb).tobytes() == got.tobytes()
    A.close(), B.close()


# ---- 3. drivers
@pytest.mark.parametrize("first_id", oc.FIRST_IDS)
def test_row_overlaps_does_not_depend_on_pool_or_window(ctx, hand_made, every, first_id):
    ix, src = hand_made[first_id]
    ka, kb, want = oc.named_pairs()
    extra = np.random.Generator(np.random.PCG64(3)).integers(0, oc.N * oc.N, size=150)
    ka, kb, want = np.concatenate([ka, every[0][extra]]), np.concatenate([kb, every[1][extra]]), np.concatenate([want, every[2][extra]])
    a, b = first_id + ka.astype(np.int64), first_id + kb.astype(np.int64)
    n_a, n_b = (np.array([len(oc.ROWS[k]) for k in x], np.uint32) for x in (ka, kb))
    distinct = len(np.unique(ka)) + len(np.unique(kb))
    host = indexio.row_overlaps_host(src + (oc.N, first_id), None, a, b, window=16, pool_hashes=5000, threads=2)
    assert np.array_equal(host[0], want)
    for pool in POOLS:
        for window in WINDOWS:
            st = {}
            got = indexio.row_overlaps(ix, None, a, b, window=window, pool_hashes=pool, stats=st)
            assert all(np.array_equal(g, h) and g.dtype == np.uint32 for g, h in zip(got, host)), (pool, window)
            assert np.array_equal(got[1], n_a) and np.array_equal(got[2], n_b)
            assert st["distinct"] == distinct and st["extractions"] >= distinct and (pool < (1 << 40) or st["extractions"] == distinct)
    other = hand_made[5 if first_id == 0 else 0][0]                               # two indices
    got = indexio.row_overlaps(ix, other, a, other.first_id + kb.astype(np.int64), window=7, pool_hashes=9000)
    assert np.array_equal(got[0], want)
    assert all(len(x) == 0 for x in indexio.row_overlaps(ix, None, [], []))


# ---- 4. a built index pins the meaning
def test_built_index_equals_the_hasher(ctx):
    import folddisco_amd as fd
    from folddisco_amd import synth
    ps = synth.to_packed(synth.generate(180, seed=31))
    off = ps.res_off.astype(np.int64)
    items = [dict(n_xyz=ps.n_xyz[off[s]:off[s + 1]], ca_xyz=ps.ca_xyz[off[s]:off[s + 1]], cb_xyz=ps.cb_xyz[off[s]:off[s + 1]], aa=ps.aa[off[s]:off[s + 1]])
             for s in range(ps.n_struct)]
    h, ho = fd.get_geometric_hash_as_u32(ctx, ctx.upload(ps), sort_dedup=True)
    row = lambda s: h[int(ho[s]):int(ho[s + 1])]
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(ps), first_id=7)
    pick = np.arange(20, 60)
    a, b = (x.ravel() for x in np.meshgrid(pick, pick, indexing="ij"))
    a, b = a[a < b], b[a < b]
    assert len(a) == 780
    inter, n_a, n_b = indexio.row_overlaps(ix, None, 7 + a, 7 + b, window=16, pool_hashes=60000)
    want = np.array([len(np.intersect1d(row(x), row(y))) for x, y in zip(a, b)], np.uint32)
    assert np.array_equal(inter, want) and want.max() > 0
    assert np.array_equal(n_a, [len(row(x)) for x in a]) and np.array_equal(n_b, [len(row(y)) for y in b])
    # a second index over the same 40 structures: every copy overlaps its original in all of its hashes
    copy = fd.FolddiscoIndex.build(ctx, ctx.upload(fd.PackedStructures.concat(items[20:60])), first_id=0)
    j = np.arange(40)
    inter, n_a, n_b = indexio.row_overlaps(ix, copy, 7 + 20 + j, j, window=8)
    assert np.array_equal(inter, n_a) and np.array_equal(inter, n_b) and np.array_equal(inter, [len(row(20 + k)) for k in j]) and inter.min() > 0
    inter, _, _ = indexio.row_overlaps(ix, copy, 7 + 20 + j, j[::-1].copy())       # and the other pairs as inside one index
    assert np.array_equal(inter, [len(np.intersect1d(row(20 + k), row(59 - k))) for k in j])


# ---- 5. refusals
def test_refusals_leave_everything_as_it_was(ctx, hand_made):
    ix, _ = hand_made[5]
    L = ctx.L
    ctx.enable_timing(True)
    A, _ = ix.rowset(5 + np.arange(10))
    before = [n for n, _, _ in ctx.last_timings()]
    assert "rowset_gather" in before and "rows_plan" in before

    def rowset(ids, n=None, window=0):
        out, taken = C.c_void_p(1), C.c_uint64(9)
        arr = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
        rc = L.fdgpu_index_rowset(ctx.h, ix.h, None if arr is None else arr.ctypes.data_as(u32p), len(arr) if n is None else n, window, 0, C.byref(out), C.byref(taken))
        return rc, out.value, L.fdgpu_last_error(ctx.h).decode()

    def intersect(ka, kb, n=None, B=None):
        out = u32p()
        out.contents = C.c_uint32(7)
        arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.uint32).ctypes.data_as(u32p)
        rc = L.fdgpu_rowset_intersect(ctx.h, A.h, B, arr(ka), arr(kb), len(ka) if n is None else n, C.byref(out))
        return rc, bool(out), L.fdgpu_last_error(ctx.h).decode()
    for ids, n in (([6, 6], None), ([8, 7], None), ([4], None), ([5 + oc.N], None), ([5, 5 + oc.N], None), (None, 3), ([5], 1 << 32)):
        rc, out, msg = rowset(ids, n)
        assert (rc, out) == (-1, None) and msg.startswith("index rowset:"), (ids, msg)
        assert [n_ for n_, _, _ in ctx.last_timings()] == before
    for ka, kb, n in (([10], [0], None), ([0], [10], None), (None, [0], 1), ([0], None, 1), ([0], [0], 1 << 32)):
        rc, out, msg = intersect(ka, kb, n)
        assert (rc, out) == (-1, False) and msg.startswith("rowset intersect:"), (ka, kb, msg)
        assert [n_ for n_, _, _ in ctx.last_timings()] == before
    # the context works afterwards; empty id and pair lists are valid
    assert ctx.rowset_intersect(A, None, [3, 9], [3, 2]).tolist() == [len(oc.ROWS[3]), len(oc.SETS[9] & oc.SETS[2])]
    assert [n for n, _, _ in ctx.last_timings()][-2:] == ["overlap_pairs", "overlap_copy"]
    E, taken = ix.rowset([])
    assert (taken, E.n_rows, E.n_hashes) == (0, 0, 0) and len(E.export()[0]) == 0 and E.export()[1].tolist() == [0]
    assert len(ctx.rowset_intersect(A, None, [], [])) == 0 and len(ctx.rowset_intersect(E, None, [], [])) == 0
    rc, out, msg = intersect([0], [0], B=E.h)                                     # no row in an empty set
    assert (rc, out) == (-1, False) and msg.startswith("rowset intersect:")
    ctx.enable_timing(False)
    A.close(), E.close()


# ---- 6. commands
def test_overlap_command_equals_host(tmp_path, capsys):
    one, two, dev, host, pf = (str(tmp_path / n) for n in ("one", "two", "dev.tsv", "host.tsv", "pairs.txt"))
    tids = write_index(one)
    tids2 = write_index(two, tids=[f"u{k}" for k in range(oc.N)])
    ka, kb, _ = oc.named_pairs()
    with open(pf, "w") as f:
        f.writelines(f"{tids[a]}\t{tids[b]}\n" for a, b in zip(ka, kb))
    capsys.readouterr()
    assert _status(["overlap", "-i", one, "--pairs", pf, "-o", dev, "--verify", "-v", "--window", "5", "--min-jaccard", "0.3"]) == 0
    cap = capsys.readouterr()
    assert _status(["overlap", "--host", "-i", one, "--pairs", pf, "-o", host, "--min-jaccard", "0.3"]) == 0
    assert capsys.readouterr().out == cap.out and "[INFO] overlap on the device" in cap.err
    assert open(dev).read() == open(host).read() and 0 < open(dev).read().count("\n") < len(ka)
    with open(pf, "w") as f:
        f.writelines(f"{tids[a]}\t{tids2[b]}\n" for a, b in zip(ka, kb))
    assert _status(["overlap", "-i", one, "--against", two, "--pairs", pf, "-o", dev, "--pool-mb", "1"]) == 0
    assert _status(["overlap", "--host", "-i", one, "--against", two, "--pairs", pf, "-o", host]) == 0
    assert open(dev).read() == open(host).read() and open(dev).read().count("\n") == len(ka)
    names = sorted(os.listdir(tmp_path))
    assert _status(["overlap", "-i", one, "--pairs", pf, "-o", dev]) == 1                      # tid_b names no row of the first index
    assert _status(["overlap", "-i", one, "--pairs", pf, "-o", dev, "--min-jaccard", "0"]) == 1
    assert _status(["overlap", "-i", one, "--pairs", str(tmp_path / "nope"), "-o", dev]) == 2
    assert _status(["overlap", "-i", str(tmp_path / "nope"), "--pairs", pf, "-o", dev]) == 2
    assert sorted(os.listdir(tmp_path)) == names


def test_min_jaccard_commands_equal_host_and_feed_update(tmp_path, capsys):
    one, dev, host, red, red_h, conf = (str(tmp_path / n) for n in ("one", "dev.tsv", "host.tsv", "red.txt", "red_host.txt", "confirm.tsv"))
    tids = write_index(one)
    where = {t: k for k, t in enumerate(tids)}
    F = 0.9
    assert _status(["dups", "-i", one, "-o", conf, "--confirm", "--min-similarity", "0.3"]) == 0
    assert _status(["dups", "-i", one, "-o", dev, "--min-jaccard", str(F), "--min-similarity", "0.3", "--window", "9"]) == 0
    assert _status(["dups", "--host", "-i", one, "-o", host, "--min-jaccard", str(F), "--min-similarity", "0.3"]) == 0
    all_rows = open(conf).readlines()
    want = [l for l in all_rows if _reaches(l.split("\t")[1], l.split("\t")[4], where, F)]
    assert 0 < len(want) < len(all_rows) and open(dev).readlines() == want == open(host).readlines()
    capsys.readouterr()
    assert _status(["cluster", "-i", one, "-o", dev, "--min-jaccard", str(F), "--redundant", red, "--min-similarity", "0.5"]) == 0
    line = capsys.readouterr().out
    assert _status(["cluster", "--host", "-i", one, "-o", host, "--min-jaccard", str(F), "--redundant", red_h, "--min-similarity", "0.5"]) == 0
    assert capsys.readouterr().out == line and "members below the exact floor kept" in line
    assert open(dev).read() == open(host).read() and open(red).read() == open(red_h).read()
    members = [l.split("\t") for l in open(dev).readlines() if l.split("\t")[9] != "representative"]
    reach = sorted((int(m[3]), m[4]) for m in members if _reaches(m[1], m[4], where, F))
    assert 0 < len(reach) < len(members) and open(red).read().split() == [t for _, t in reach]
    # what the list is for
    out = str(tmp_path / "nr")
    assert _status(["update", "-i", one, "--remove", red, "-o", out]) == 0
    assert _status(["verify", "-i", out]) == 0
    left = [r.split("\t")[1] for r in indexio.read_lookup_rows(out + ".lookup")]
    assert left == [t for t in tids if t not in {t for _, t in reach}]
