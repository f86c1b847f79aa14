"""Seeded signature clusters on the CPU (fdgpu_signature_clusters_seeded_host, indexio.signature_clusters_host(seeds=...)): the host form and
indexio.signature_clusters_from_tables equal an independent brute force byte for byte on the grid of drops and seed tables, for every
threshold and walk order; seedless calls equal the unseeded form; the concatenation property against the unseeded form; the planted cases in
three placements; thread counts; the refusals through ctypes and Python; `cluster --host --against` with its files and refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from folddisco_amd import _lib, indexio
from tests import cluster_cases as cc
from tests import seeded_cluster_cases as scc
from tests.test_index_signatures_host import N, _jaccard, _status, _write_index, lists, no_device      # noqa: F401

DT = indexio.SIGNATURE_NEIGHBOR_DTYPE
SDT = indexio.SIGNATURE_DTYPE


def test_the_layouts_of_the_cases_are_the_products():
    assert scc.SDT == SDT and scc.DT == DT and (scc.IDENTICAL, scc.SEED) == (indexio.SIG_IDENTICAL, indexio.SIG_SEED) == (1, 2)


@pytest.mark.parametrize("n", scc.NS)
def test_host_equals_brute_force_and_the_numpy_definition(n):
    for nT in scc.NTS:
        S, T = scc.grid_tables(n, nT)
        void = T.copy()
        void["n"] = 0                                                          # seeds with empty rows and full sketches: never candidates
        for thr in scc.THRESHOLDS:
            for name in scc.ORDERS:
                order = cc.order_of(S, name)
                w = scc.want(n, nT, thr, name)
                got = indexio.signature_clusters_host(S, order, thr64=thr, threads=2, seeds=T)
                assert got.dtype == DT and got.shape == (n,)
                for f in DT.names:
                    assert np.array_equal(got[f], w[f]), (n, nT, thr, name, f)
                assert got.tobytes() == w.tobytes()
                if name in ("identity", "random"):
                    assert indexio.signature_clusters_from_tables(S, order, thr, seeds=T).tobytes() == w.tobytes(), (n, nT, thr, name)
                plain = indexio.signature_clusters_host(S, order, thr64=thr)
                if nT == 0:
                    assert got.tobytes() == plain.tobytes() and got.tobytes() == cc.brute_clusters(S, order, thr, DT).tobytes()
                assert indexio.signature_clusters_host(S, order, thr64=thr, seeds=void).tobytes() == plain.tobytes(), (n, nT, thr, name)
            assert indexio.signature_clusters_host(S, None, thr64=thr, seeds=T).tobytes() == scc.want(n, nT, thr, "identity").tobytes()
        assert indexio.signature_clusters_from_tables(S, None, 48, seeds=void).tobytes() == indexio.signature_clusters_from_tables(S, None, 48).tobytes()


@pytest.mark.parametrize("cell", ((513, 700), (257, 65), (1, 700)))
def test_threads_do_not_change_the_result(cell):
    S, T = scc.grid_tables(*cell)
    for thr, name in ((48, "random"), (1, "reverse")):
        for threads in (1, 3, 8):
            got = indexio.signature_clusters_host(S, cc.order_of(S, name), thr64=thr, threads=threads, seeds=T)
            assert got.tobytes() == scc.want(*cell, thr, name).tobytes(), (cell, thr, name, threads)


def test_invariants_of_a_seeded_result():
    """a member carries the pair values with what it joined, which stood before it; no new representative is a reported pair with a seed or
    with another one"""
    n, nT, thr = 513, 257, 48
    S, T = scc.grid_tables(n, nT)
    order = cc.order_of(S, "random")
    got = indexio.signature_clusters_host(S, order, thr64=thr, seeds=T)
    of_seed, rep, of_new = scc.kinds(got)
    assert of_seed.sum() > 50 and rep.sum() > 50 and of_new.sum() > 10
    assert len(indexio.signature_pairs_host(S[rep], thr64=thr)) == 0 and len(indexio.signature_pairs_host(S[rep], T, thr64=thr)) == 0
    match, filled = scc.matrices(S, np.concatenate([T, S]))
    place = np.empty(n, np.int64)
    place[order.astype(np.int64)] = np.arange(n)
    for p in np.nonzero(of_seed | of_new)[0]:
        r = int(got["id"][p])
        x = r if of_seed[p] else nT + r
        assert (int(got["match"][p]), int(got["filled"][p])) == (match[p, x], filled[p, x]) and match[p, x] * 64 >= thr * filled[p, x] > 0
        assert of_seed[p] and T["n"][r] > 0 or rep[r] and place[r] < place[p]


@pytest.mark.parametrize("cell", scc.CONCAT_CELLS)
def test_concatenation_property(cell):
    """the unseeded walk of [A; B], A first, is the seeded walk of B against A's representatives"""
    n, nT = cell
    Bt, A = scc.grid_tables(n, nT)
    oA, oB, joined_order = scc.concat_orders(A, Bt)
    for thr in (32, 48):
        joined = indexio.signature_clusters_host(np.concatenate([A, Bt]), joined_order, thr64=thr)
        RA, w = scc.concat_expected(joined, nT, DT)
        assert 0 < len(RA) <= nT and (w["flags"] & scc.SEED).any()
        got = indexio.signature_clusters_host(Bt, oB, thr64=thr, threads=2, seeds=A[RA])
        assert got.tobytes() == w.tobytes(), (cell, thr)
        assert indexio.signature_clusters_from_tables(Bt, oB, thr, seeds=A[RA]).tobytes() == w.tobytes(), (cell, thr)


def _pair_values(S, T):
    """match and filled of the planted positions 3, 7 and 299 of S with every combined id, indexed by position"""
    m, f = scc.matrices(S[[3, 7, 299]], np.concatenate([T, S]))
    return dict(zip(((p, x) for p in (3, 7, 299) for x in range(m.shape[1])), m.ravel().tolist())), \
        dict(zip(((p, x) for p in (3, 7, 299) for x in range(f.shape[1])), f.ravel().tolist()))


def test_planted_cases():
    cases = scc.planted_want()
    assert len(cases) == 3 * 9
    for name, S, T, order, thr, expect, w in cases:
        assert scc.named(w, expect) == expect, name                            # the case is what it claims to be
        got = indexio.signature_clusters_host(S, order, thr64=thr, threads=2, seeds=T)
        assert got.tobytes() == w.tobytes(), name
        assert indexio.signature_clusters_from_tables(S, order, thr, seeds=T).tobytes() == w.tobytes(), name
    by = {c[0]: c for c in cases}
    for how in scc.PLACEMENTS:
        _, S, T, _, _, _, _ = by[f"tie_seed_wins_{how}"]
        m, f = _pair_values(S, T)
        assert (m[299, 650], f[299, 650]) == (m[299, 700 + 3], f[299, 700 + 3]) == (48, 64)
        _, S, T, _, _, _, _ = by[f"new_nearer_{how}"]
        m, f = _pair_values(S, T)
        assert (m[299, 700 + 3], m[299, 650], m[3, 650]) == (52, 44, 32)
        _, S, T, _, _, _, w = by[f"paired_seeds_{how}"]
        m, f = _pair_values(S, T)
        assert (m[299, 3], m[299, 300], m[7, 300], m[7, 3]) == (56, 56, 62, 54)
        assert len(indexio.signature_pairs_host(T[[3, 300]], thr64=48)) == 1       # the two seeds are a reported pair
        _, S, T, _, _, _, _ = by[f"filled_seed_{how}"]
        m, f = _pair_values(S, T)
        assert (m[299, 650], f[299, 650], m[299, 700 + 3], f[299, 700 + 3]) == (30, 40, 24, 32)
        _, S, T, _, _, _, w = by[f"empty_seed_{how}"]
        assert T["n"][650] == 0 and (T["sk"][650] == S["sk"][3]).all() and w["flags"][299] == 1


def test_refusals():
    S, T = scc.grid_tables(65, 64)
    L = _lib.load()
    good = np.arange(65, dtype=np.uint32)

    def call(tab, n, order, seeds, nT, thr):
        out = C.c_void_p(1)
        rc = L.fdgpu_signature_clusters_seeded_host(tab, n, None if order is None else order.ctypes.data, seeds, nT, thr, 1, C.byref(out))
        return rc, out.value
    s, t = S.ctypes.data, T.ctypes.data
    for thr in (0, 65, 1 << 31):
        assert call(s, 65, good, t, 64, thr) == (-1, None)
    assert call(s, 1 << 32, None, t, 64, 32) == (-1, None)
    assert call(None, 3, None, t, 64, 32) == (-1, None)
    assert call(s, 65, None, None, 64, 32) == (-1, None)                       # a NULL seed table with a count
    assert call(s, 65, None, t, 0xffffffff - 64, 32) == (-1, None)             # nT + n = 2^32: the combined ids would reach 0xFFFFFFFF
    assert call(s, 65, None, t, 1 << 32, 32) == (-1, None)
    twice, beyond = good.copy(), good.copy()
    twice[7] = 8
    beyond[64] = 65
    assert call(s, 65, twice, t, 64, 32) == (-1, None) and call(s, 65, beyond, t, 64, 32) == (-1, None)
    rc, p = call(None, 0, None, t, 64, 32)                                     # n == 0: an empty result, one record's room
    assert rc == 0 and p
    L.fdgpu_free(C.c_void_p(p))
    rc, p = call(s, 65, good[::-1].copy(), None, 0, 64)                        # no seeds: T may be NULL
    assert rc == 0 and p
    L.fdgpu_free(C.c_void_p(p))
    for kw in (dict(thr64=0), dict(thr64=65), dict(order=twice), dict(order=good[:5])):
        with pytest.raises(ValueError, match="^signature clusters:"):
            indexio.signature_clusters_host(S, seeds=T, **kw)
        with pytest.raises(ValueError, match="^signature clusters:"):
            indexio.signature_clusters_from_tables(S, seeds=T, **kw)
    for bad in (np.zeros(3, np.uint32), np.zeros((2, 2), SDT)):
        with pytest.raises(ValueError, match="^seeds:"):
            indexio.signature_clusters_host(S, seeds=bad)
        with pytest.raises(ValueError, match="^seeds:"):
            indexio.signature_clusters_from_tables(S, seeds=bad)
    assert indexio.signature_clusters_host(S[:0], seeds=T).shape == (0,) and indexio.signature_clusters_from_tables(S[:0], seeds=T).shape == (0,)


# ---- the command, on the CPU: the files rebuilt from the brute force, and the refusals before any device call
N_DB = 30


def _rows_of(lists, parts):
    out = np.zeros(len(parts) + 1, np.uint64)
    out[1:] = np.cumsum([len(p) for p in parts])
    return np.concatenate(parts), out


def _db_and_drop(lists):
    """DB: the first 30 structures of the hand-made batch.  DROP: the ten others, then copies of the DB's 3 and 17, its 5 less one hash, a copy
    of the drop's own 3 (structure 33), its 5 less two hashes, and an empty row"""
    h, off = lists
    row = lambda k: h[int(off[k]):int(off[k + 1])]
    db = _rows_of(lists, [row(k) for k in range(N_DB)])
    drop = _rows_of(lists, [row(k) for k in range(N_DB, N)] + [row(3), row(17), row(5)[:-1], row(33), row(35)[:-2], row(0)[:0]])
    return db, drop


def _expected(db, drop, tdb, tdrop, thr64, seed_ids=None, confirm=False, by="hashes"):
    """the command's files and last line from the Python forms alone: signatures_from_rows, the brute force, a set Jaccard"""
    S, S2 = indexio.signatures_from_rows(*drop), indexio.signatures_from_rows(*db)
    seed_ids = np.arange(len(S2)) if seed_ids is None else np.asarray(seed_ids)
    n = len(S)
    key = {"hashes": S["n"].astype(np.int64), "id": -np.arange(n)}[by]
    order = np.array(sorted(range(n), key=lambda k: (-int(key[k]), k)), np.uint32)
    cl = scc.brute_seeded(S, order, thr64, S2[seed_ids], DT)
    of_seed, rep, of_new = scc.kinds(cl)
    rep_id = [int(seed_ids[cl["id"][p]]) if of_seed[p] else int(cl["id"][p]) for p in range(n)]
    rows = []
    row = lambda ls, k: ls[0][int(ls[1][k]):int(ls[1][k + 1])]
    for p in sorted((p for p in range(n) if cl["id"][p] != cc.NO_ID), key=lambda p: (not of_seed[p], rep_id[p], p)):
        r = rep_id[p]
        kind = "representative" if rep[p] else "identical" if cl["flags"][p] & 1 else "similar"
        rt, rs, rl = (tdb, S2, db) if of_seed[p] else (tdrop, S, drop)
        cols = [str(r), rt[r], str(int(rs["n"][r])), str(p), tdrop[p], str(int(S["n"][p])), str(int(cl["match"][p])), str(int(cl["filled"][p])),
                f"{int(cl['match'][p]) / max(int(cl['filled'][p]), 1):.4f}", kind, "against" if of_seed[p] else "self"]
        if confirm:
            cols.append("1.0000" if rep[p] else f"{_jaccard(row(rl, r), row(drop, p)):.4f}")
        rows.append("\t".join(cols) + "\n")
    singles = sum(1 for p in range(n) if rep[p] and not any(of_new[q] and cl["id"][q] == p for q in range(n)))
    member = of_seed | of_new
    return "".join(rows), cl, (f"{n} x {len(S2)} structures, {len(seed_ids)} seeds, {int(rep.sum())} new clusters ({singles} singletons), {int(of_seed.sum())} members "
                               f"of seeds, {int(of_new.sum())} members of new representatives ({int((member & ((cl['flags'] & 1) != 0)).sum())} identical), "
                               f"{int((cl['id'] == cc.NO_ID).sum())} unclustered, threshold {thr64}/64\n")


def test_cluster_against_host_command(tmp_path, lists, no_device, capsys):
    dbp, dropp, out, red, reps = (str(tmp_path / f) for f in ("db", "drop", "OUT.tsv", "redundant.txt", "reps.txt"))
    db, drop = _db_and_drop(lists)
    n = len(drop[1]) - 1
    tdb, tdrop = [f"s{k}" for k in range(N_DB)], [f"d{k}" for k in range(n)]
    _write_index(dbp, db, tdb)
    _write_index(dropp, drop, tdrop)
    assert _status(["cluster", "--host", "-i", dropp, "--against", dbp, "-o", out, "--redundant", red, "--representatives", reps, "-t", "3", "--verify", "-v",
                    "--min-similarity", "0.5"]) == 0
    cap = capsys.readouterr()
    text, cl, tail = _expected(db, drop, tdb, tdrop, 32)
    assert open(out).read() == text
    assert cap.out == f"[OK] {dropp} x {dbp}: " + tail and f"{N_DB} seeds of {dbp} (0 of them with empty rows)" in cap.err
    of_seed, rep, of_new = scc.kinds(cl)
    assert (int(cl["id"][10]), int(cl["id"][11]), int(cl["id"][12])) == (3, 17, 5) and of_seed[10] and of_seed[11] and of_seed[12] and cl["flags"][10] == 3
    assert int(cl["id"][13]) == 3 and of_new[13] and cl["flags"][13] == 1 and int(cl["id"][14]) == 5 and of_new[14] and cl["id"][15] == cc.NO_ID
    assert "\tagainst\n" in text and "\tself\n" in text and text.index("\tself\n") > text.rindex("\tagainst\n")
    assert open(red).read() == "".join(tdrop[p] + "\n" for p in range(n) if of_seed[p] or of_new[p])
    assert open(reps).read() == "".join(tdrop[p] + "\n" for p in range(n) if rep[p])
    # --min-jaccard gates the removal list for both kinds of members: the copies stay listed, the structures less a hash or two are kept
    assert _status(["cluster", "--host", "-i", dropp, "--against", dbp, "-o", out, "--redundant", red, "--min-similarity", "0.5", "--min-jaccard", "1.0"]) == 0
    cap = capsys.readouterr()
    row = lambda ls, k: ls[0][int(ls[1][k]):int(ls[1][k + 1])]
    exact = {p: _jaccard(row(db if of_seed[p] else drop, int(cl["id"][p])), row(drop, p)) for p in range(n) if of_seed[p] or of_new[p]}
    listed = [p for p in sorted(exact) if exact[p] == 1.0]
    assert {10, 11, 13} <= set(listed) and 12 not in listed and 14 not in listed
    assert open(red).read() == "".join(tdrop[p] + "\n" for p in listed)
    assert cap.out == f"[OK] {dropp} x {dbp}: " + tail[:-1] + f", {len(exact) - len(listed)} members below the exact floor kept\n"
    assert open(out).read() == "".join(l[:-1] + "\t" + ("1.0000" if rep[int(l.split("\t")[3])] else f"{exact[int(l.split(chr(9))[3])]:.4f}") + "\n" for l in text.splitlines(True))
    # standard output, the default threshold, --confirm, another walk and a seed list: the DB's 3 is no seed, so its copy is new
    listed = str(tmp_path / "seeds.txt")
    seed_ids = [k for k in range(N_DB) if k != 3]
    with open(listed, "w") as f:
        f.write("".join(f"s{k}\n" for k in reversed(seed_ids)) + "\ns17\n")
    assert _status(["cluster", "--host", "-i", dropp, "--against", dbp, "--against-reps", listed, "--confirm", "--rep-by", "id", "--window", "7"]) == 0
    cap = capsys.readouterr()
    text, cl, tail = _expected(db, drop, tdb, tdrop, 58, seed_ids=seed_ids, confirm=True, by="id")
    assert cap.out == text + f"[OK] {dropp} x {dbp}: " + tail
    assert int(cl["id"][10]) == 10 and cl["flags"][10] == 1 and seed_ids[int(cl["id"][11])] == 17 and cl["flags"][11] == 3
    assert "\n17\ts17\t" in text and all(l.split("\t")[11] == "1.0000" for l in text.splitlines() if l.split("\t")[9] in ("representative", "identical"))
    # without --against the rows have no rep_from column, and --representatives lists the representatives
    assert _status(["cluster", "--host", "-i", dropp, "-o", out, "--representatives", reps, "--min-similarity", "0.5"]) == 0
    plain = indexio.signature_clusters_host(indexio.signatures_from_rows(*drop), cc.order_of(indexio.signatures_from_rows(*drop), "n_descending"), thr64=32)
    assert all(len(l.split("\t")) == 10 for l in open(out).read().splitlines())
    assert open(reps).read() == "".join(tdrop[p] + "\n" for p in range(n) if plain["id"][p] == p)
    assert not [f for f in os.listdir(tmp_path) if "cluster-tmp" in f]


def test_cluster_against_refusals_before_any_device_call(tmp_path, lists, no_device, capsys):
    dbp, dropp, out, red, reps = (str(tmp_path / f) for f in ("db", "drop", "OUT.tsv", "redundant.txt", "reps.txt"))
    db, drop = _db_and_drop(lists)
    n = len(drop[1]) - 1
    _write_index(dbp, db, [f"s{k}" for k in range(N_DB)])
    _write_index(dropp, drop, [f"d{k}" for k in range(n)])
    other, twice = str(tmp_path / "other"), str(tmp_path / "twice")
    _write_index(other, db, [f"s{k}" for k in range(N_DB)], nbin_dist=8)
    _write_index(twice, db, ["s0"] + [f"s{k}" for k in range(N_DB - 1)])   # the tid s0 names two rows
    for ext in ("", ".offset", ".lookup", ".type"):
        with open(str(tmp_path / "sh") + ".shard0of2" + ext, "wb") as f:
            f.write(open(dbp + ext, "rb").read())
    unknown, dup, fine = (str(tmp_path / f) for f in ("unknown.txt", "dup.txt", "fine.txt"))
    with open(unknown, "w") as f:
        f.write("s1\n" + "".join(f"x{k}\n" for k in range(12)))
    with open(dup, "w") as f:
        f.write("s0\ns5\n")
    with open(fine, "w") as f:
        f.write("s1\ns2\n")
    names = sorted(os.listdir(tmp_path))
    capsys.readouterr()
    base = ["cluster", "-i", dropp, "-o", out, "--redundant", red, "--representatives", reps]
    assert _status(base + ["--against", dropp]) == 2 and _status(base + ["--against", str(tmp_path / "." / "drop")]) == 2      # the index itself: status 2
    capsys.readouterr()
    assert _status(base + ["--against", other]) == 1 and "num_bin_dist" in capsys.readouterr().out
    assert _status(base + ["--against", str(tmp_path / "sh")]) == 1 and "sharded" in capsys.readouterr().out
    assert _status(base + ["--against", str(tmp_path / "nope")]) == 2
    assert _status(base + ["--against-reps", fine]) == 1                       # --against-reps without --against
    assert _status(base + ["--against", dbp, "--against-reps", str(tmp_path / "nope.txt")]) == 2
    capsys.readouterr()
    assert _status(base + ["--against", dbp, "--against-reps", unknown]) == 1
    msg = capsys.readouterr().out
    assert "12 tid(s)" in msg and "x0, x1, x2, x3, x4, x5, x6, x7, x8, x9 ..." in msg and "x10" not in msg
    assert _status(base + ["--against", twice, "--against-reps", dup]) == 1
    msg = capsys.readouterr().out
    assert "1 tid(s)" in msg and "s0" in msg and "more than one row" in msg
    for x in ("0", "nan"):
        assert _status(base + ["--against", dbp, "--min-similarity", x]) == 1
    assert _status(base + ["--against", dbp, "--rep-by", "tid"]) == 1
    assert sorted(os.listdir(tmp_path)) == names
