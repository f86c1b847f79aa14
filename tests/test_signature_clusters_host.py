"""Signature clusters on the CPU (fdgpu_signature_clusters_host, indexio.signature_clusters_host): the host form equals an independent brute
force and indexio.signature_clusters_from_tables byte for byte on the hand-made tables, for every size, threshold and walk order; the
invariants of the definition, the planted cases in both placements, thread counts, the refusals, and `cluster --host` with its refusals.

Case (d) of the planted cases reads "24/32 against 48/64" in the request.  One signature cannot hold both: match <= the buckets filled in
both and filled >= its own filled buckets, so 48 matches need 48 filled buckets and then no partner gives filled = 32.  The case is built
with the same ratio as 24/32 against 30/40 (cluster_cases.planted), which decides by `filled` in the same way."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from folddisco_amd import _lib, indexio
from tests import cluster_cases as cc
from tests import signature_cases as sc

DT = indexio.SIGNATURE_NEIGHBOR_DTYPE
SDT = indexio.SIGNATURE_DTYPE


@functools.lru_cache(maxsize=None)
def table(n):
    return cc.table(n, SDT)


@functools.lru_cache(maxsize=None)
def want(n, thr, order):
    """the brute force, computed once per case and left alone"""
    S = table(n)
    return cc.brute_clusters(S, cc.order_of(S, order), thr, DT)


def _invariants(S, order, thr, got):
    """no two representatives are a reported pair; every member carries the pair values with its representative, which was walked before it;
    empty rows are unclustered"""
    ids = np.arange(len(S))
    reps = ids[got["id"] == ids]
    assert len(sc.brute_pairs(S[reps], None, thr, indexio.SIGNATURE_PAIR_DTYPE)) == 0
    place = np.empty(len(S), np.int64)
    place[np.asarray(order, np.int64)] = ids
    match, filled = cc.matrices(S)
    for p in ids[(got["id"] != ids) & (got["id"] != cc.NO_ID)]:
        r = int(got["id"][p])
        assert got["id"][r] == r and place[r] < place[p]
        same = S["n"][r] == S["n"][p] and S["d0"][r] == S["d0"][p] and S["d1"][r] == S["d1"][p]
        assert (int(got["match"][p]), int(got["filled"][p]), int(got["flags"][p])) == (match[p, r], filled[p, r], int(same))
        assert match[p, r] * 64 >= thr * filled[p, r] > 0
    none = got["id"] == cc.NO_ID
    assert np.array_equal(none, S["n"] == 0) and not got["match"][none].any() and not got["filled"][none].any() and not got["flags"][none].any()
    assert (got["flags"][reps] == 1).all() and np.array_equal(got["match"][reps], (S["sk"][reps] != cc.EMPTY).sum(-1))
    assert np.array_equal(got["match"][reps], got["filled"][reps])


@pytest.mark.parametrize("n", cc.SIZES)
def test_host_equals_brute_force_and_the_numpy_definition(n):
    S = table(n)
    for thr in cc.THRESHOLDS:
        for name in cc.ORDERS:
            order = cc.order_of(S, name)
            w = want(n, thr, name)
            got = indexio.signature_clusters_host(S, order, thr64=thr)
            assert got.dtype == DT and got.shape == (n,)
            for f in DT.names:
                assert np.array_equal(got[f], w[f]), (n, thr, name, f)
            assert got.tobytes() == w.tobytes()
            assert indexio.signature_clusters_from_tables(S, order, thr).tobytes() == w.tobytes(), (n, thr, name)
            for threads in (1, 3, 8):
                assert indexio.signature_clusters_host(S, order, thr64=thr, threads=threads).tobytes() == w.tobytes(), (n, thr, name, threads)
            _invariants(S, order, thr, got)
        assert indexio.signature_clusters_host(S, None, thr64=thr).tobytes() == want(n, thr, "identity").tobytes()      # no order: position order


@pytest.mark.parametrize("n", cc.HOST_SIZES)
def test_host_blocks_and_threads(n):
    """tables that straddle the host form's block of 1,024 positions: the scan of the representatives of earlier blocks, and (2,049) enough of
    them that the threads asked for are really started"""
    S = table(n)
    ids = np.arange(n)
    for thr, name in ((48, "random"), (32, "identity")):
        order = cc.order_of(S, name)
        w = want(n, thr, name)
        place = np.empty(n, np.int64)
        place[order.astype(np.int64)] = ids
        member = (w["id"] != ids) & (w["id"] != cc.NO_ID)
        across = member & (place[np.where(member, w["id"], 0)] // cc.HOST_B < place // cc.HOST_B)
        assert n > cc.HOST_B or not across.any()
        if n > 2 * cc.HOST_B:                                                  # members whose representative is in an earlier host block, and a
            before = int(((w["id"] == ids) & (place < cc.HOST_B)).sum())       # second block with work for more than three threads
            assert across.sum() > 100 and cc.HOST_B * before >= 4 * cc.HOST_THREAD_WORK, (n, thr, name, before)
        for threads in (1, 3, 8):
            got = indexio.signature_clusters_host(S, order, thr64=thr, threads=threads)
            assert got.tobytes() == w.tobytes(), (n, thr, name, threads)
        assert indexio.signature_clusters_from_tables(S, order, thr).tobytes() == w.tobytes(), (n, thr, name)
        _invariants(S, order, thr, got)


def test_the_tables_exercise_what_they_should():
    for n in (257, 700):
        S = table(n)
        ids = np.arange(n)
        w = want(n, 48, "identity")
        reps = int((w["id"] == ids).sum())
        assert reps > 64 and (w["id"] == cc.NO_ID).sum() >= 2 and ((w["id"] != ids) & (w["id"] != cc.NO_ID)).sum() > 20
        assert (w["flags"][w["id"] != ids] & 1).any()                          # a member identical with its representative
        assert want(n, 48, "reverse").tobytes() != w.tobytes() and want(n, 1, "identity").tobytes() != w.tobytes()
    w = want(700, 48, "identity")
    later = [p for p in range(700) if w["id"][p] not in (p, cc.NO_ID) and w["id"][p] // cc.B == p // cc.B]
    earlier = [p for p in range(700) if w["id"][p] not in (p, cc.NO_ID) and w["id"][p] // cc.B < p // cc.B]
    assert later and earlier                                                   # representatives inside a member's block and before it
    got = indexio.signature_clusters_host(table(700), thr64=48)
    assert got[later].tobytes() == w[later].tobytes() and got[earlier].tobytes() == w[earlier].tobytes()


def test_the_extreme_tables():
    R = cc.all_random(SDT)
    ids = np.arange(len(R))
    for thr in cc.THRESHOLDS:
        for order in (None, ids[::-1].astype(np.uint32)):
            got = indexio.signature_clusters_host(R, order, thr64=thr, threads=3)
            assert np.array_equal(got["id"], ids) and (got["match"] == 64).all() and (got["flags"] == 1).all()
            assert got.tobytes() == cc.brute_clusters(R, order, thr, DT).tobytes()
    K = cc.all_copies(SDT)
    for thr in cc.THRESHOLDS:
        got = indexio.signature_clusters_host(K, None, thr64=thr, threads=3)
        assert (got["id"] == 0).all() and (got["match"] == 64).all() and (got["filled"] == 64).all() and (got["flags"] == 1).all()
        order = np.roll(ids, -123).astype(np.uint32)                           # position 123 is walked first
        assert (indexio.signature_clusters_host(K, order, thr64=thr)["id"] == 123).all()


@functools.lru_cache(maxsize=None)
def planted():
    return cc.planted(SDT)


def test_planted_cases():
    cases = planted()
    assert len(cases) == 2 * (2 + 3 * 4) + 1
    for name, S, order, thr, expect in cases:
        w = cc.brute_clusters(S, order, thr, DT)
        assert {p: int(w["id"][p]) for p in expect} == expect, name            # the case is what it claims to be
        got = indexio.signature_clusters_host(S, order, thr64=thr, threads=2)
        assert got.tobytes() == w.tobytes(), name
        assert indexio.signature_clusters_from_tables(S, order, thr).tobytes() == w.tobytes(), name
        _invariants(S, order, thr, got)
    by = {c[0]: c for c in cases}
    for tag in ("far", "near"):
        _, S, _, _, _ = by[f"tie_P50_walk0_{tag}"]
        m, f = cc.matrices(S)
        assert (m[299, 50], f[299, 50]) == (m[299, 450], f[299, 450]) == (48, 64)
        _, S, _, _, _ = by[f"filled_P50_walk0_{tag}"]
        m, f = cc.matrices(S)
        assert (m[299, 50], f[299, 50], m[299, 450], f[299, 450]) == (30, 40, 24, 32)
        _, S, _, _, _ = by[f"nearest_P450_walk1_{tag}"]
        m, f = cc.matrices(S)
        assert (m[299, 450], m[299, 50], m[450, 50]) == (52, 44, 32)
    _, S, order, _, _ = by["empties"]
    assert S["n"][5] == 0 and (S["sk"][5] != cc.EMPTY).all() and (S["sk"][5] == S["sk"][444]).all()


def test_min_similarity_is_the_threshold():
    S = table(257)
    assert indexio.signature_clusters_host(S, min_similarity=0.5).tobytes() == want(257, 32, "identity").tobytes()
    assert indexio.signature_clusters_host(S).tobytes() == cc.brute_clusters(S, None, 58, DT).tobytes()      # the default: 0.9
    assert indexio.signature_clusters_from_tables(S).tobytes() == cc.brute_clusters(S, None, 58, DT).tobytes()
    assert indexio.signature_clusters_host(S[:0]).shape == (0,) and indexio.signature_clusters_from_tables(S[:0]).shape == (0,)


def test_refusals():
    S = table(65)
    L = _lib.load()
    good = np.arange(65, dtype=np.uint32)

    def call(tab, n, order, thr):
        out = C.c_void_p(1)
        rc = L.fdgpu_signature_clusters_host(tab, n, None if order is None else order.ctypes.data, thr, 1, C.byref(out))
        return rc, out.value
    s = S.ctypes.data
    for thr in (0, 65, 1 << 31):
        assert call(s, 65, good, thr) == (-1, None)
    assert call(s, 1 << 32, None, 32) == (-1, None)                          # refused before anything is read
    assert call(None, 3, None, 32) == (-1, None)                             # a NULL table with a count
    twice, beyond = good.copy(), good.copy()
    twice[7] = 8
    beyond[64] = 65
    assert call(s, 65, twice, 32) == (-1, None) and call(s, 65, beyond, 32) == (-1, None)
    assert call(s, 64, good[1:].copy(), 32) == (-1, None)                    # the value 64 in an order of 64
    rc, p = call(None, 0, None, 32)                                          # n == 0: an empty result, one record's room
    assert rc == 0 and p
    L.fdgpu_free(C.c_void_p(p))
    rc, p = call(s, 65, good[::-1].copy(), 64)
    assert rc == 0 and p
    L.fdgpu_free(C.c_void_p(p))
    for kw in (dict(thr64=0), dict(thr64=65), dict(thr64=-1), dict(order=twice), dict(order=beyond), dict(order=good[:5]), dict(order=good.astype(np.float64))):
        with pytest.raises(ValueError, match="^signature clusters:"):
            indexio.signature_clusters_host(S, **kw)
    for kw in (dict(thr64=0), dict(thr64=65), dict(order=twice), dict(order=good[:5])):
        with pytest.raises(ValueError, match="^signature clusters:"):
            indexio.signature_clusters_from_tables(S, **kw)


def test_cluster_order():
    S = table(65)
    rows = [f"{k}\tt{k}\t{100 + k % 7}\t{50 + (k * 5) % 11}.5\n" for k in range(65)]
    ids = np.arange(65)
    assert np.array_equal(indexio.cluster_order(S, rows, "id"), ids)
    assert indexio.cluster_order(S, rows, "id").dtype == np.uint32
    for by, key in (("hashes", S["n"].astype(np.int64)), ("nres", 100 + ids % 7), ("plddt", (ids * 5) % 11)):
        want_ = sorted(range(65), key=lambda k: (-int(key[k]), k))
        assert indexio.cluster_order(S, rows, by).tolist() == want_, by
    assert np.array_equal(indexio.cluster_order(S, rows, "hashes"), cc.order_of(S, "n_descending"))
    with pytest.raises(ValueError, match="unknown representative key"):
        indexio.cluster_order(S, rows, "tid")
    with pytest.raises(ValueError):
        indexio.cluster_order(S, rows[:3], "nres")


# ---- the command, on the CPU: the file rebuilt from the brute force, and the refusals before any device call
from tests.test_index_signatures_host import N, _jaccard, _status, _write_index, lists, no_device      # noqa: E402,F401


def _family(lists):
    """the hand-made index's rows with a family planted: 40 .. 42 are structure 5 less one, two and three hashes, 43 is a copy of structure 9,
    44 an empty row"""
    h, off = lists
    row = lambda k: h[int(off[k]):int(off[k + 1])]
    parts = [row(k) for k in range(N)] + [row(5)[:-1], row(5)[:-2], row(5)[3:], row(9), row(0)[:0]]
    out = np.zeros(len(parts) + 1, np.uint64)
    out[1:] = np.cumsum([len(p) for p in parts])
    return np.concatenate(parts), out


def _expected(ls, tids, thr64, by="hashes", confirm=False, nres=None):
    S = indexio.signatures_from_rows(*ls)
    n = len(S)
    key = {"hashes": S["n"].astype(np.int64), "nres": nres, "id": -np.arange(n)}[by]
    order = np.array(sorted(range(n), key=lambda k: (-int(key[k]), k)), np.uint32)
    cl = cc.brute_clusters(S, order, thr64, DT)
    rows = []
    for p in sorted((p for p in range(n) if cl["id"][p] != cc.NO_ID), key=lambda p: (int(cl["id"][p]), p)):
        r = int(cl["id"][p])
        kind = "representative" if r == p else "identical" if cl["flags"][p] & 1 else "similar"
        cols = [str(r), tids[r], str(int(S["n"][r])), str(p), tids[p], str(int(S["n"][p])), str(int(cl["match"][p])), str(int(cl["filled"][p])),
                f"{int(cl['match'][p]) / max(int(cl['filled'][p]), 1):.4f}", kind]
        if confirm:
            cols.append("1.0000" if r == p else f"{_jaccard(ls[0][int(ls[1][r]):int(ls[1][r + 1])], ls[0][int(ls[1][p]):int(ls[1][p + 1])]):.4f}")
        rows.append("\t".join(cols) + "\n")
    return "".join(rows), cl


def _last_line(prefix, cl, thr64):
    ids = np.arange(len(cl))
    rep = cl["id"] == ids
    member = ~rep & (cl["id"] != cc.NO_ID)
    sizes = np.bincount(cl["id"][rep | member].astype(np.int64), minlength=len(cl))
    return (f"[OK] {prefix}: {len(cl)} structures, {int(rep.sum())} clusters ({int((sizes[rep] == 1).sum())} singletons), {int(member.sum())} members "
            f"({int((member & ((cl['flags'] & 1) != 0)).sum())} identical), {int((cl['id'] == cc.NO_ID).sum())} unclustered, "
            f"largest cluster {int(sizes.max()) if len(cl) else 0}, threshold {thr64}/64\n")


def test_cluster_host_command(tmp_path, lists, no_device, capsys):
    one, out, red = str(tmp_path / "one"), str(tmp_path / "OUT.tsv"), str(tmp_path / "redundant.txt")
    ls = _family(lists)
    n = len(ls[1]) - 1
    tids = [f"s{k}" for k in range(n)]
    _write_index(one, ls, tids)
    assert _status(["cluster", "--host", "-i", one, "-o", out, "--redundant", red, "-t", "3", "--verify", "-v", "--min-similarity", "0.5"]) == 0
    cap = capsys.readouterr()
    want_, cl = _expected(ls, tids, 32)
    assert open(out).read() == want_
    assert cap.out == _last_line(one, cl, 32) and "[INFO] cluster on the host" in cap.err
    assert int(cl["id"][40]) == 5 and int(cl["id"][41]) == 5 and int(cl["id"][42]) == 5 and cl["id"][44] == cc.NO_ID
    assert {int(cl["id"][9]), int(cl["id"][43])} == {9} and (cl["flags"][43] & 1) and "\tidentical" in want_ and "\tsimilar" in want_
    members = [p for p in range(n) if cl["id"][p] not in (p, cc.NO_ID)]
    assert open(red).read() == "".join(tids[p] + "\n" for p in members) and {40, 41, 42, 43} <= set(members)
    # standard output, the default threshold, with --confirm and another walk
    assert _status(["cluster", "--host", "-i", one, "--confirm", "--rep-by", "id", "--window", "7"]) == 0
    cap = capsys.readouterr()
    want_, cl = _expected(ls, tids, 58, by="id", confirm=True)
    assert cap.out == want_ + _last_line(one, cl, 58)
    assert all(l.split("\t")[10] == "1.0000" for l in want_.splitlines() if l.split("\t")[9] in ("representative", "identical"))
    assert int(cl["id"][5]) == 5 and int(cl["id"][40]) == 5                      # walked by id, 5 represents its family
    # --rep-by nres: _write_index gives structure k 50 + k residues, so the walk is the reverse of the ids
    assert _status(["cluster", "--host", "-i", one, "-o", out, "--rep-by", "nres", "--min-similarity", "0.5"]) == 0
    want_, cl = _expected(ls, tids, 32, by="nres", nres=50 + np.arange(n))
    assert open(out).read() == want_ and int(cl["id"][5]) in (40, 41, 42) and int(cl["id"][9]) == 43
    capsys.readouterr()
    assert _status(["cluster", "--host", "-i", one, "-o", out, "--rep-by", "plddt", "--min-similarity", "0.5"]) == 0      # one plddt everywhere: by id
    assert open(out).read() == _expected(ls, tids, 32, by="id")[0]
    assert not [f for f in os.listdir(tmp_path) if "cluster-tmp" in f]


def test_cluster_refusals_before_any_device_call(tmp_path, lists, no_device, capsys):
    one, out, red = str(tmp_path / "one"), str(tmp_path / "OUT.tsv"), str(tmp_path / "redundant.txt")
    ls = _family(lists)
    n = len(ls[1]) - 1
    _write_index(one, ls, [f"s{k}" for k in range(n)])
    shared = str(tmp_path / "shared")                                         # the member 40 has the tid of a representative, the member 41 that of the empty row 44
    tids = [f"s{k}" for k in range(n)]
    cl = _expected(ls, tids, 32)[1]
    kept = next(p for p in range(n) if cl["id"][p] == p and p != 5)
    assert cl["id"][40] == 5 and cl["id"][41] == 5 and cl["id"][44] == cc.NO_ID
    tids[40], tids[41] = tids[kept], tids[44]
    _write_index(shared, ls, tids)
    bad = str(tmp_path / "bad")
    _write_index(bad, ls, [f"s{k}" for k in range(n)])
    with open(bad, "ab") as f:
        f.write(b"\x01")
    for ext in ("", ".offset", ".lookup", ".type"):                           # a sharded prefix: no single index
        with open(str(tmp_path / "sh") + ".shard0of2" + ext, "wb") as f:
            f.write(open(one + ext, "rb").read())
    names = sorted(os.listdir(tmp_path))
    capsys.readouterr()
    for x in ("0", "-0.5", "1.01", "nan"):
        assert _status(["cluster", "-i", one, "-o", out, "--min-similarity", x]) == 1
    assert _status(["cluster", "-i", one, "-o", out, "--window", "0"]) == 1
    capsys.readouterr()
    assert _status(["cluster", "-i", one, "-o", out, "--rep-by", "tid"]) == 1 and "tid" in capsys.readouterr().out
    assert _status(["cluster", "-i", bad, "-o", out]) == 1 and "inconsistent" in capsys.readouterr().out
    assert _status(["cluster", "-i", str(tmp_path / "sh"), "-o", out]) == 1 and "sharded" in capsys.readouterr().out
    assert _status(["cluster", "-i", str(tmp_path / "nope"), "-o", out]) == 2
    with pytest.raises(SystemExit) as e:                                      # there is no --against
        from folddisco_amd.__main__ import main
        main(["cluster", "-i", one, "--against", one])
    assert e.value.code == 2
    capsys.readouterr()
    # --redundant names a tid that a kept row carries too: refused, nothing written (on the host, where the clusters are known)
    assert _status(["cluster", "--host", "-i", shared, "-o", out, "--redundant", red, "--min-similarity", "0.5"]) == 1
    msg = capsys.readouterr().out
    assert f"s{kept}" in msg and "s44" in msg and "2 tid" in msg
    assert sorted(os.listdir(tmp_path)) == names
    assert _status(["cluster", "--host", "-i", shared, "-o", out, "--min-similarity", "0.5"]) == 0      # without --redundant the same index is served
    assert os.path.exists(out) and not os.path.exists(red)
