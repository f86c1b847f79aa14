"""Exact neighbours on the CPU, no GPU: fdgpu_rows_neighbors_host (indexio.rows_neighbors_host) equals the plain statement
(indexio.row_neighbors_from_rows: Python sets and a full sort) on the hand-made rows for every first id, k, floor and thread count; the tiling
driver row_neighbors_host gives one result for every pool and window; the refusals; `neighbors --exact --host` with its TSV, last line and
refusals, none of which opens a device; plain `neighbors --host` writes what it wrote before."""
import ctypes as C
import os

import numpy as np
import pytest

from folddisco_amd import _lib, indexio
from tests import exact_neighbor_cases as xc

POOLS = (2, 5000, 1 << 40)
WINDOWS = (1, 16, 16384)
u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def files():
    return {f: xc.index(f) + (xc.S, f) for f in xc.FIRST_IDS}


@pytest.fixture
def no_device(monkeypatch):
    import folddisco_amd as fd

    def boom(*a, **k):
        raise AssertionError("a device was touched by a host-side command or before its validation ended")
    monkeypatch.setattr(fd, "Context", boom)


def test_statement_has_the_planted_answers():
    where = {int(k): j for j, k in enumerate(xc.QUERIES)}
    got = xc.statement(0, 32, 0)
    assert got.dtype == indexio.ROW_NEIGHBOR_DTYPE and got.shape == (len(xc.QUERIES), 32)
    for q in (xc.NAMES["tie_q"], xc.NAMES["hub33"], xc.NAMES["hub9"], xc.NAMES["leaf32"], 43, 1, xc.NAMES["len1000"]):
        want = xc.ranked(q)[:32]
        row = got[where[q]]
        assert [(int(r["inter"]), int(r["union"]), int(r["id"])) for r in row[:len(want)]] == want
        assert all(int(r["id"]) == indexio.ROW_NO_ID and not (int(r["inter"]) | int(r["union"]) | int(r["flags"])) for r in row[len(want):])
    assert (got[where[43]]["flags"][:3] == [1, 1, 0]).all() and got[where[xc.NAMES["twin594"]]]["flags"][0] == 1
    assert (got[where[0]]["id"] == indexio.ROW_NO_ID).all() and (got[where[xc.NAMES["len1"]]]["id"] == indexio.ROW_NO_ID).all()
    # a floor keeps a prefix of the order; at 10000 only equal rows are left
    top = xc.statement(0, 8, 10000)
    assert {int(k) for j, k in enumerate(xc.QUERIES) if int(top[j, 0]["id"]) != indexio.ROW_NO_ID} == {41, 42, 43, 44, 45, 46, 47, 594, 595}
    assert (top["flags"][top["id"] != indexio.ROW_NO_ID] == 1).all()


@pytest.mark.parametrize("first_id", xc.FIRST_IDS)
def test_host_form_equals_the_statement(files, first_id):
    q_rows = xc.rows_csr(xc.QUERIES)
    ex = (first_id + xc.QUERIES).astype(np.uint32)
    for k in xc.KS:
        for T in xc.FLOORS:
            want = xc.statement(first_id, k, T)
            for threads in (1, 3, 8):
                got = indexio.rows_neighbors_host(q_rows, files[first_id], xc.LENGTHS, k=k, floor_e4=T, exclude=ex, threads=threads)
                assert got.dtype == indexio.ROW_NEIGHBOR_DTYPE and got.tobytes() == want.tobytes(), (k, T, threads)
    # without the exclusion a non-empty row is its own nearest, identical; a floor given as a fraction is the same floor
    got = indexio.rows_neighbors_host(q_rows, files[first_id], xc.LENGTHS, k=8, threads=2)
    assert got.tobytes() == xc.statement(first_id, 8, 0, exclude_self=False).tobytes()
    full = xc.LENGTHS[xc.QUERIES] > 0
    assert (got["flags"][full, 0] == 1).all() and (got["inter"][full, 0] == xc.LENGTHS[xc.QUERIES][full]).all()
    assert indexio.rows_neighbors_host(q_rows, files[first_id], xc.LENGTHS, k=8, floor=0.5, exclude=ex).tobytes() == xc.statement(first_id, 8, 5000).tobytes()
    assert indexio.rows_neighbors_host(xc.csr([]), files[first_id], xc.LENGTHS, k=8).shape == (0, 8)


def test_against_reaches_beyond_the_hashes_of_the_index(files):
    """query rows of the second index against the lists of the first, and the other way round: hashes below the first hash of the lists, above
    the last, 0 and 0xFFFFFFFF themselves, hashes in no list"""
    ag = xc.against_index() + (len(xc.AGAINST_ROWS), xc.AGAINST_FIRST)
    q_ag, q_d = xc.csr(xc.AGAINST_ROWS), xc.rows_csr(xc.QUERIES)
    ag_len = np.array([len(r) for r in xc.AGAINST_ROWS], np.uint32)
    for k in (1, 32):
        for T in (0, 5000):
            want = indexio.row_neighbors_from_rows(q_ag, xc.rows_csr(), 16200, k, T, None)
            assert indexio.rows_neighbors_host(q_ag, files[16200], xc.LENGTHS, k=k, floor_e4=T, threads=3).tobytes() == want.tobytes()
            back = indexio.row_neighbors_from_rows(q_d, q_ag, xc.AGAINST_FIRST, k, T, None)
            assert indexio.rows_neighbors_host(q_d, ag, ag_len, k=k, floor_e4=T, threads=2).tobytes() == back.tobytes()
    want = indexio.row_neighbors_from_rows(q_ag, xc.rows_csr(), 16200, 32, 0, None)
    assert all((want[j]["id"] == indexio.ROW_NO_ID).all() for j in (1, 2, 3, 4, 7))
    assert want[5, 0]["flags"] == 1 and want[5, 0]["id"] == 16200 + xc.NAMES["len64"] and (want[0]["id"] != indexio.ROW_NO_ID).all()


@pytest.mark.parametrize("first_id", xc.FIRST_IDS)
def test_driver_does_not_depend_on_pool_or_window(files, first_id):
    ids = first_id + xc.QUERIES
    ex = ids.astype(np.uint32)
    want = xc.statement(first_id, 8, 1)
    for pool in POOLS:
        for window in WINDOWS:
            st = {}
            got = indexio.row_neighbors_host(files[first_id], None, ids, xc.LENGTHS, k=8, floor_e4=1, exclude=ex, window=window, pool_hashes=pool, threads=2, stats=st)
            assert got.tobytes() == want.tobytes(), (pool, window)
            assert (st["chunks"] == 1) == (pool == 1 << 40) and (pool != 2 or st["chunks"] > len(ids) // 2)      # a pool of 2: a row a chunk, but for rows of 0 or 1
    ag = xc.against_index() + (len(xc.AGAINST_ROWS), xc.AGAINST_FIRST)
    got = indexio.row_neighbors_host(ag, files[first_id], xc.AGAINST_FIRST + np.arange(40), xc.LENGTHS, k=32, pool_hashes=300, window=7)
    assert got.tobytes() == indexio.row_neighbors_from_rows(xc.csr(xc.AGAINST_ROWS), xc.rows_csr(), first_id, 32, 0, None).tobytes()
    assert indexio.row_neighbors_host(files[first_id], None, [], xc.LENGTHS, k=4).shape == (0, 4)
    for bad in ([first_id + 5, first_id + 5], [first_id + 6, first_id + 5], [first_id + xc.S], [first_id - 1] if first_id else [-1]):
        with pytest.raises(ValueError):
            indexio.row_neighbors_host(files[first_id], None, bad, xc.LENGTHS, k=4)


def test_host_refusals(files):
    v, h, o, S, first = files[16200]
    qh, qo = xc.rows_csr([1, 43, 0])
    L = _lib.load()
    arr = lambda x, t, dt: None if x is None else np.ascontiguousarray(x, dtype=dt).ctypes.data_as(t)

    def call(k=8, T=0, d_len=xc.LENGTHS, exclude=None, q_off=qo, q_hashes=qh, nQ=3, value=v, offsets=o, out=True, first_id=first):
        op = C.c_void_p(1)
        rc = L.fdgpu_rows_neighbors_host(arr(q_hashes, u32p, np.uint32), arr(q_off, u64p, np.uint64), nQ, arr(h, u32p, np.uint32), arr(offsets, u64p, np.uint64), len(h),
                                         arr(value, u8p, np.uint8), len(value), first_id, S, arr(d_len, u32p, np.uint32), arr(exclude, u32p, np.uint32), k, T, 1,
                                         C.byref(op) if out else None)
        return rc, op.value
    rc, op = call()
    assert rc == 0 and op
    L.fdgpu_free(C.c_void_p(op))
    for kw in (dict(k=0), dict(k=33), dict(T=10001), dict(d_len=None), dict(q_off=None), dict(q_hashes=None), dict(exclude=[16199, 0xFFFFFFFF, 0xFFFFFFFF]),
               dict(exclude=[16200 + xc.S, 0xFFFFFFFF, 0xFFFFFFFF]), dict(exclude=[0, 16200, 16200]), dict(q_off=qo[::-1].copy()), dict(first_id=0xFFFFFFFF)):
        assert call(**kw) == (-1, None), kw
    assert call(out=False)[0] == -1
    rc, op = call(exclude=[0xFFFFFFFF, 16200, 16200 + xc.S - 1])
    assert rc == 0 and op
    L.fdgpu_free(C.c_void_p(op))
    # row lengths that are not the index's: one entry lowered, and a twin of that structure asks
    low = xc.LENGTHS.copy()
    low[44] -= 1
    assert call(d_len=low) == (-1, None)
    with pytest.raises(ValueError, match="^row neighbors:"):
        indexio.rows_neighbors_host((qh, qo), files[16200], low, k=8)
    # a damaged index is an error: an id at first_id + S in one list, offsets that descend, a list that ends inside a varint
    bad_v, bad_h, bad_o = xc.damaged_index(16200)
    assert np.array_equal(bad_h, h) and call(value=bad_v, offsets=bad_o) == (-1, None)
    t = int(np.searchsorted(h, xc.ROWS[43][5]))
    swapped = o.copy()
    swapped[t], swapped[t + 1] = o[t + 1], o[t]
    assert call(offsets=swapped) == (-1, None)
    cut = v.copy()
    cut[int(o[t + 1]) - 1] |= 0x80
    assert call(value=cut) == (-1, None)
    for kw in (dict(k=0), dict(k=33), dict(floor_e4=10001), dict(floor=0.0), dict(floor=1.5), dict(exclude=[1, 2]), dict(exclude=[5, 16200, 16200])):
        with pytest.raises(ValueError):
            indexio.rows_neighbors_host((qh, qo), files[16200], xc.LENGTHS, **kw)
    with pytest.raises(ValueError, match="^row neighbors:"):
        indexio.rows_neighbors_host((qh, qo), files[16200], xc.LENGTHS[:-1])


def test_neighbors_exact_host_command(tmp_path, no_device, capsys):
    one, two, out, tf = (str(tmp_path / n) for n in ("one", "two", "OUT.tsv", "tids.txt"))
    tids = xc.write_index(one)
    tids2 = xc.write_index(two, rows=xc.AGAINST_ROWS, tids=[f"u{k}" for k in range(40)])
    every = np.arange(xc.S)
    ag_len = [len(r) for r in xc.AGAINST_ROWS]
    capsys.readouterr()
    assert xc.status(["neighbors", "--exact", "--host", "-i", one, "-o", out, "-t", "3", "--verify", "--window", "50", "--pool-mb", "1"]) == 0
    nb = xc.statement(0, 8, 0, queries=every)
    assert open(out).read() == xc.exact_tsv(nb, every, tids, tids, xc.LENGTHS, xc.LENGTHS)
    rows, none, ident = int((nb["id"] != indexio.ROW_NO_ID).sum()), int((nb["id"][:, 0] == indexio.ROW_NO_ID).sum()), int((nb["flags"][:, 0] & 1).sum())
    assert none == 6 and ident == 9                   # four empty rows, `lone` and `len1`; the nine twins
    assert capsys.readouterr().out == f"[OK] {one}: 600 structures, k = 8, exact, {rows} rows, {none} without a neighbour, {ident} with an identical nearest, floor 0/10000\n"
    # a floor, k = 32, chosen queries, standard output
    asked = [xc.NAMES[n] for n in ("hub33", "tie_q", "twin44", "empty300", "len1000", "fam1_7")]
    with open(tf, "w") as f:
        f.writelines(f"{tids[k]}\n" for k in asked)
    assert xc.status(["neighbors", "--exact", "--host", "-i", one, "--tids", tf, "-k", "32", "--min-jaccard", "0.02", "-v"]) == 0
    cap = capsys.readouterr()
    ids = np.array(sorted(asked))
    nb = xc.statement(0, 32, 200, queries=ids)
    want = xc.exact_tsv(nb, ids, tids, tids, xc.LENGTHS, xc.LENGTHS)
    rows, none, ident = want.count("\n"), int((nb["id"][:, 0] == indexio.ROW_NO_ID).sum()), int((nb["flags"][:, 0] & 1).sum())
    assert 0 < rows < 6 * 32 and none == 1 and ident == 1
    assert cap.out == want + f"[OK] {one}: 600 structures, k = 32, exact, {rows} rows, 1 without a neighbour, 1 with an identical nearest, floor 200/10000\n"
    assert "[INFO] neighbors --exact on the host: 6 queries against 600 structures" in cap.err
    # --against: the queries of the small index among the structures of the large one, and the other way round; nothing is excluded
    assert xc.status(["neighbors", "--exact", "--host", "-i", two, "--against", one, "-o", out, "-k", "1"]) == 0
    nb = indexio.row_neighbors_from_rows(xc.csr(xc.AGAINST_ROWS), xc.rows_csr(), 0, 1, 0, None)
    assert open(out).read() == xc.exact_tsv(nb, np.arange(40), tids2, tids, ag_len, xc.LENGTHS)
    rows, none = int((nb["id"] != indexio.ROW_NO_ID).sum()), int((nb["id"][:, 0] == indexio.ROW_NO_ID).sum())
    assert none == 5 and int((nb["flags"][:, 0] & 1).sum()) == 3      # the copies of len64, tie_q and hub9
    assert capsys.readouterr().out == f"[OK] {two} x {one}: 40 x 600 structures, k = 1, exact, {rows} rows, {none} without a neighbour, 3 with an identical nearest, floor 0/10000\n"
    assert xc.status(["neighbors", "--exact", "--host", "-i", one, "--against", two, "-o", out, "--tids", tf, "--min-jaccard", "1e-4", "--counter-mb", "1"]) == 0
    nb = indexio.row_neighbors_from_rows(xc.rows_csr(ids), xc.csr(xc.AGAINST_ROWS), 0, 8, 1, None)
    assert open(out).read() == xc.exact_tsv(nb, ids, tids, tids2, xc.LENGTHS, ag_len) and "floor 1/10000" in capsys.readouterr().out
    assert not [f for f in os.listdir(tmp_path) if "neighbors-tmp" in f]


def test_neighbors_exact_refusals_and_the_plain_command(tmp_path, no_device, capsys):
    one, out, plain, flagged = (str(tmp_path / n) for n in ("one", "OUT.tsv", "plain.tsv", "flagged.tsv"))
    sub = xc.ROWS[30:70] + xc.ROWS[585:600]
    tids = xc.write_index(one, rows=sub)
    names = sorted(os.listdir(tmp_path))
    capsys.readouterr()
    assert xc.status(["neighbors", "--host", "-i", one, "-o", out, "--min-jaccard", "0.5"]) == 1                      # the floor of --exact without it
    assert xc.status(["neighbors", "--host", "--exact", "-i", one, "-o", out, "--confirm"]) == 1
    assert xc.status(["neighbors", "--host", "--exact", "-i", one, "-o", out, "--min-similarity", str(1.0 / 64)]) == 1      # explicit, even at the default's value
    for x in ("0", "-0.5", "1.01", "nan"):
        assert xc.status(["neighbors", "--host", "--exact", "-i", one, "-o", out, "--min-jaccard", x]) == 1
    assert xc.status(["neighbors", "--host", "--exact", "-i", one, "-o", out, "-k", "33"]) == 1
    assert xc.status(["neighbors", "--host", "--exact", "-i", one, "-o", out, "--pool-mb", "0"]) == 1
    assert xc.status(["neighbors", "--host", "--exact", "-i", one, "-o", out, "--counter-mb", "0"]) == 1
    assert xc.status(["neighbors", "--host", "--exact", "-i", str(tmp_path / "nope"), "-o", out]) == 2
    assert sorted(os.listdir(tmp_path)) == names
    capsys.readouterr()
    # without --exact: the bytes of the command as it was, whether or not the new size flags are given
    assert xc.status(["neighbors", "--host", "-i", one, "-o", plain, "-k", "5", "--confirm"]) == 0
    line = capsys.readouterr().out
    assert xc.status(["neighbors", "--host", "-i", one, "-o", flagged, "-k", "5", "--confirm", "--pool-mb", "4096", "--counter-mb", "7"]) == 0
    assert capsys.readouterr().out == line and open(plain).read() == open(flagged).read()
    A = np.array(indexio.signatures_host(*xc._index_of(sub, 0), len(sub)))
    nb = indexio.signature_neighbors_from_tables(A, None, k=5, thr64=1)
    lines = []
    for q in range(len(sub)):
        for rank, r in enumerate(nb[q]):
            if int(r["id"]) == indexio.SIG_NO_ID:
                break
            s = int(r["id"])
            i = len(set(sub[q]) & set(sub[s]))
            lines.append("\t".join([str(q), tids[q], str(len(sub[q])), str(rank + 1), str(s), tids[s], str(len(sub[s])), str(int(r["match"])), str(int(r["filled"])),
                                    f"{int(r['match']) / int(r['filled']):.4f}", "identical" if int(r["flags"]) & 1 else "similar",
                                    f"{i / max(len(set(sub[q]) | set(sub[s])), 1):.4f}"]) + "\n")
    assert open(plain).read() == "".join(lines) and len(lines) > 40
    n_none, n_ident = int((nb["id"][:, 0] == indexio.SIG_NO_ID).sum()), int((nb["flags"][:, 0] & 1).sum())
    assert line == f"[OK] {one}: {len(sub)} structures, k = 5, {len(lines)} rows, {n_none} without a neighbour, {n_ident} with an identical nearest, floor 1/64\n"
