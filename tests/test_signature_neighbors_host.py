"""Signature neighbours on the CPU (fdgpu_signature_neighbors_host, indexio.signature_neighbors_host): the host form equals a numpy brute force
and indexio.signature_neighbors_from_tables field by field on the hand-made tables, for every size, k and threshold, inside one table and
between two; thread counts, the exclusion, empty tables, k beyond the table, the refusals, and the order of every row."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from folddisco_amd import _lib, indexio
from tests import neighbor_cases as nc

DT = indexio.SIGNATURE_NEIGHBOR_DTYPE


@functools.lru_cache(maxsize=None)
def tables(n):
    A = nc.table(n, indexio.SIGNATURE_DTYPE)
    return A, nc.other(A)


@functools.lru_cache(maxsize=None)
def want(n, two, k, thr):
    """the brute force, computed once per case; row q of the two-table mode are the neighbours of B[q] in A"""
    A, B = tables(n)
    return nc.brute_neighbors(B, A, k, thr, None, DT) if two else nc.brute_neighbors(A, None, k, thr, None, DT)


def _run(n, two, k, thr, **kw):
    A, B = tables(n)
    return indexio.signature_neighbors_host(B, A, k=k, thr64=thr, **kw) if two else indexio.signature_neighbors_host(A, k=k, thr64=thr, **kw)


def test_the_tables_exercise_what_they_should():
    """ties that only the id decides at the cut, rows that are not full, queries without a candidate, the 64 / 64 tie of records 8 and 9"""
    for n in (129, 257, 600):
        A, _ = tables(n)
        full = nc.brute_neighbors(A, None, 33, 1, None, DT)
        for k in (1, 4, 32):
            cut = full[:, k - 1:k + 1]
            tie = (cut["id"][:, 1] != nc.NO_ID) & (cut["match"][:, 0] == cut["match"][:, 1]) & (cut["filled"][:, 0] == cut["filled"][:, 1])
            assert tie.sum() >= 18, (n, k)
        filled = (full["id"] != nc.NO_ID).sum(1)
        assert ((filled > 0) & (filled < 32)).any() and (filled > 32).any() and 3 <= (filled == 0).sum() <= 9
        assert ((nc.brute_neighbors(A, None, 4, 64, None, DT)["id"] != nc.NO_ID).sum(1) == 0).mean() > 0.8
    A, _ = tables(129)
    r0 = nc.brute_neighbors(A, None, 2, 64, None, DT)[0]
    assert r0["id"].tolist() == [8, 9] and r0["match"].tolist() == [64, 64] and r0["flags"].tolist() == [1, 0]


@pytest.mark.parametrize("n", nc.SIZES)
def test_host_equals_brute_force_and_the_numpy_definition(n):
    A, B = tables(n)
    for two in (False, True):
        for k in nc.KS:
            for thr in nc.THRESHOLDS:
                w = want(n, two, k, thr)
                got = _run(n, two, k, thr)
                assert got.dtype == DT and got.shape == ((len(B) if two else n), k)
                for f in DT.names:
                    assert np.array_equal(got[f], w[f]), (n, two, k, thr, f)
                spec = indexio.signature_neighbors_from_tables(B, A, k, thr) if two else indexio.signature_neighbors_from_tables(A, None, k, thr)
                assert spec.dtype == DT and spec.tobytes() == w.tobytes(), (n, two, k, thr)
                assert got.tobytes() == _run(n, two, k, thr, threads=3).tobytes()
    assert (want(n, True, 4, 1)["flags"] & 1).any()                          # the copies of A's records in the second table


@pytest.mark.parametrize("n", (129, 600))
def test_rows_are_sorted_without_repeats_and_without_the_query(n):
    for two in (False, True):
        got = _run(n, two, 32, 1)
        for q, row in enumerate(got):
            m = int((row["id"] != nc.NO_ID).sum())
            assert (row["id"][m:] == nc.NO_ID).all() and not row["match"][m:].any() and not row["filled"][m:].any() and not row["flags"][m:].any()
            assert all(nc.nearer(row[s], row[s + 1]) for s in range(m - 1)), (n, two, q)      # strictly: no id twice
            assert len(set(row["id"][:m].tolist())) == m and (two or q not in row["id"][:m])
            assert (row["filled"][:m] > 0).all() and (row["match"][:m] > 0).all()


def test_min_similarity_is_the_threshold():
    A, _ = tables(129)
    assert indexio.signature_neighbors_host(A, k=4, min_similarity=0.5).tobytes() == want(129, False, 4, 32).tobytes()
    assert indexio.signature_neighbors_host(A, k=4).tobytes() == want(129, False, 4, 1).tobytes()      # the default floor: 1 / 64
    assert indexio.signature_neighbors_host(A).shape == (129, 8)


def test_exclude_names_the_query_in_the_full_table():
    A, _ = tables(257)
    ids = np.array([0, 8, 9, 63, 64, 200, 256, 8], np.uint32)
    for k in nc.KS:
        got = indexio.signature_neighbors_host(A[ids], A, k=k, thr64=1, exclude=ids, threads=2)
        assert got.tobytes() == want(257, False, k, 1)[ids].tobytes()
        assert got.tobytes() == nc.brute_neighbors(A[ids], A, k, 1, ids, DT).tobytes()
        assert got.tobytes() == indexio.signature_neighbors_from_tables(A[ids], A, k, 1, ids).tobytes()
    free = indexio.signature_neighbors_host(A[ids], A, k=1, thr64=1, exclude=np.full(len(ids), nc.NO_ID, np.uint32))
    assert free.tobytes() == indexio.signature_neighbors_host(A[ids], A, k=1, thr64=1).tobytes()
    assert free["id"][0, 0] == 0 and free["flags"][0, 0] == 1                # nothing excluded: record 0 finds itself
    with pytest.raises(ValueError, match="exclude"):
        indexio.signature_neighbors_host(A[ids], A, exclude=ids[:3])


def test_empty_tables_and_k_beyond_the_table():
    A, _ = tables(65)
    got = indexio.signature_neighbors_host(A[:0], A, k=4)
    assert got.shape == (0, 4) and got.dtype == DT
    assert indexio.signature_neighbors_host(A[:0], k=4).shape == (0, 4)
    none = indexio.signature_neighbors_host(A, A[:0], k=4)
    assert none.shape == (65, 4) and (none["id"] == nc.NO_ID).all() and not none["match"].any() and not none["filled"].any() and not none["flags"].any()
    few = indexio.signature_neighbors_host(A[:5], k=32)                       # k greater than nD
    assert few.tobytes() == nc.brute_neighbors(A[:5], None, 32, 1, None, DT).tobytes() and (few["id"][:, 4:] == nc.NO_ID).all()
    one = indexio.signature_neighbors_host(A[:1], k=1)
    assert one["id"].tolist() == [[nc.NO_ID]]


def test_refusals():
    A, B = tables(65)
    L = _lib.load()
    x = np.zeros(len(B), np.uint32)

    def call(Q, nQ, D, nD, excl, k, thr):
        out = C.c_void_p(1)
        rc = L.fdgpu_signature_neighbors_host(Q, nQ, D, nD, excl, k, thr, 1, C.byref(out))
        return rc, out.value
    a, b = A.ctypes.data, B.ctypes.data
    for k, thr in ((0, 1), (33, 1), (8, 0), (8, 65)):
        assert call(b, len(B), a, len(A), None, k, thr) == (-1, None)
    assert call(b, 1 << 32, a, len(A), None, 8, 1) == (-1, None) and call(b, len(B), a, 1 << 32, None, 8, 1) == (-1, None)      # refused before anything is read
    assert call(a, len(A), None, 0, x.ctypes.data, 8, 1) == (-1, None)       # exclude in self mode
    assert call(None, 3, a, len(A), None, 8, 1) == (-1, None)                # a NULL table with a count
    rc, p = call(b, len(B), a, len(A), x.ctypes.data, 32, 64)
    assert rc == 0 and p
    L.fdgpu_free(C.c_void_p(p))
    for kw in (dict(k=0), dict(k=33), dict(k=-1), dict(thr64=0), dict(thr64=65), dict(exclude=np.zeros(len(A), np.uint32))):
        with pytest.raises(ValueError, match="^signature neighbors:"):
            indexio.signature_neighbors_host(A, **kw)


# ---- the command, on the CPU: rows from the numpy definition alone, and the refusals before any device call
from tests.test_index_signatures_host import N, _jaccard, _second, _status, _write_index, lists, no_device      # noqa: E402,F401


def _expected_tsv(lq, tq, ld, td, k, thr64, ids=None, confirm=False):
    A = indexio.signatures_from_rows(*lq)
    D = A if ld is None else indexio.signatures_from_rows(*ld)
    ids = np.arange(len(A)) if ids is None else np.asarray(ids)
    nb = nc.brute_neighbors(A[ids], D, k, thr64, ids if ld is None else None, DT)
    ld, td = (lq, tq) if ld is None else (ld, td)
    rows = []
    for q, row in zip(ids, nb):
        for rank, r in enumerate(row):
            if r["id"] == nc.NO_ID:
                break
            d = int(r["id"])
            cols = [str(q), tq[q], str(int(A["n"][q])), str(rank + 1), str(d), td[d], str(int(D["n"][d])), str(int(r["match"])), str(int(r["filled"])),
                    f"{int(r['match']) / int(r['filled']):.4f}", "identical" if r["flags"] & 1 else "similar"]
            if confirm:
                cols.append(f"{_jaccard(lq[0][int(lq[1][q]):int(lq[1][q + 1])], ld[0][int(ld[1][d]):int(ld[1][d + 1])]):.4f}")
            rows.append("\t".join(cols) + "\n")
    return "".join(rows), nb


def test_neighbors_host_command(tmp_path, lists, no_device, capsys):
    one, two, out = str(tmp_path / "one"), str(tmp_path / "two"), str(tmp_path / "OUT.tsv")
    ta, tb = [f"s{k}" for k in range(N)], [f"m{k}" for k in range(6)]
    lb = _second(lists)
    _write_index(one, lists, ta)
    _write_index(two, lb, tb)
    # the drop against the database
    assert _status(["neighbors", "--host", "-i", two, "--against", one, "-k", "2", "-o", out, "-t", "3", "--verify", "-v", "--confirm"]) == 0
    cap = capsys.readouterr()
    want, nb = _expected_tsv(lb, tb, lists, ta, 2, 1, confirm=True)
    assert open(out).read() == want and [int(l.split("\t")[4]) for l in want.splitlines() if l.split("\t")[3] == "1"] == [3, 17, 30, 5, 8, 8]
    assert cap.out == f"[OK] {two} x {one}: 6 x {N} structures, k = 2, {len(want.splitlines())} rows, 0 without a neighbour, 5 with an identical nearest, floor 1/64\n"
    assert "[INFO] neighbors on the host" in cap.err
    # inside one index, on standard output, with a floor
    assert _status(["neighbors", "--host", "-i", one, "-k", "32", "--min-similarity", "0.25"]) == 0
    cap = capsys.readouterr()
    want, nb = _expected_tsv(lists, ta, None, None, 32, 16)
    none = int((nb["id"][:, 0] == nc.NO_ID).sum())
    assert cap.out == want + f"[OK] {one}: {N} structures, k = 32, {len(want.splitlines())} rows, {none} without a neighbour, 0 with an identical nearest, floor 16/64\n"
    # --tids: chosen queries against the whole index, themselves excluded
    with open(tmp_path / "tids.txt", "w") as f:
        f.write("s30\n\ns4\ns30\n")
    assert _status(["neighbors", "--host", "-i", one, "-k", "3", "-o", out, "--tids", str(tmp_path / "tids.txt")]) == 0
    want, _ = _expected_tsv(lists, ta, None, None, 3, 1, ids=[4, 30])
    assert open(out).read() == want and want == "".join(l + "\n" for l in _expected_tsv(lists, ta, None, None, 3, 1)[0].splitlines() if l.split("\t")[0] in ("4", "30"))
    assert not [f for f in os.listdir(tmp_path) if "neighbors-tmp" in f]


def test_neighbors_refusals_before_any_device_call(tmp_path, lists, no_device, capsys):
    one, two, out = str(tmp_path / "one"), str(tmp_path / "two"), str(tmp_path / "OUT.tsv")
    _write_index(one, lists, [f"s{k}" for k in range(N)])
    _write_index(two, _second(lists), [f"m{k}" for k in range(6)])
    other = str(tmp_path / "other")
    _write_index(other, _second(lists), [f"m{k}" for k in range(6)], nbin_dist=8)
    for ext in ("", ".offset", ".lookup", ".type"):                                                   # a sharded prefix: no single index
        with open(str(tmp_path / "sh") + ".shard0of2" + ext, "wb") as f:
            f.write(open(two + ext, "rb").read())
    with open(tmp_path / "tids.txt", "w") as f:
        f.write("s3\nnobody\n")
    names = sorted(os.listdir(tmp_path))
    capsys.readouterr()
    for x in ("0", "-0.5", "1.01", "nan"):
        assert _status(["neighbors", "-i", one, "-o", out, "--min-similarity", x]) == 1               # outside (0, 1]
    for k in ("0", "33"):
        assert _status(["neighbors", "-i", one, "-o", out, "-k", k]) == 1
    assert _status(["neighbors", "-i", one, "--against", one, "-o", out]) == 1                        # --against equal to -i
    capsys.readouterr()
    assert _status(["neighbors", "-i", one, "--against", other, "-o", out]) == 1 and "num_bin_dist" in capsys.readouterr().out
    assert _status(["neighbors", "-i", str(tmp_path / "sh"), "-o", out]) == 1 and "sharded" in capsys.readouterr().out
    assert _status(["neighbors", "-i", one, "-o", out, "--tids", str(tmp_path / "tids.txt")]) == 1 and "nobody" in capsys.readouterr().out
    assert _status(["neighbors", "-i", one, "-o", out, "--tids", str(tmp_path / "none.txt")]) == 2
    assert _status(["neighbors", "-i", str(tmp_path / "nope"), "-o", out]) == 2                       # missing files
    assert _status(["neighbors", "-i", one, "--against", str(tmp_path / "nope"), "-o", out]) == 2
    assert sorted(os.listdir(tmp_path)) == names
