"""Exact row overlaps on the CPU, no GPU: fdgpu_rows_intersect_host (indexio.rows_intersect_host), the numpy statement
(indexio.row_overlaps_from_rows) and Python sets agree on the hand-made rows; the tiling driver row_overlaps_host gives one result for every
pool and window; the integer floor jaccard_reaches at its edges; `overlap --host` with its refusals, `dups --host --min-jaccard` and
`cluster --host --min-jaccard`, none of which opens a device."""
import ctypes as C
import os

import numpy as np
import pytest

from folddisco_amd import _lib, indexio
from tests import overlap_cases as oc

POOLS = (2, 5000, 20000, 1 << 40)
WINDOWS = (1, 16, 16384)


@pytest.fixture(scope="module")
def every():
    """all 4,096 ordered pairs and their expectation by Python sets, once"""
    ka, kb = oc.all_pairs()
    return ka, kb, oc.expected(ka, kb)


@pytest.fixture(scope="module")
def files():
    return {f: oc.index(f) + (oc.N, f) for f in oc.FIRST_IDS}


@pytest.fixture
def no_device(monkeypatch):
    import folddisco_amd as fd

    def boom(*a, **k):
        raise AssertionError("a device was touched by a host-side command or before its validation ended")
    monkeypatch.setattr(fd, "Context", boom)


def _status(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


def write_index(prefix, first_id=0, tids=None, **type_kw):
    """the hand-made index as files; first_id does not reach the files (a single index starts at 0)"""
    v, h, o = oc.index(0)
    indexio.write_index_files(prefix, v, h, o)
    tids = tids or [f"t{k}" for k in range(oc.N)]
    indexio.save_lookup_py(prefix + ".lookup", tids, 50 + np.arange(oc.N, dtype=np.uint64), np.full(oc.N, 80.5, np.float32))
    indexio.save_type(prefix + ".type", oc.N, **type_kw)
    return tids


def test_cases_have_the_shape(every):
    assert len(oc.U) == 9000 and oc.U == sorted(set(oc.U)) and {0, 1, oc.TOP - 1, oc.TOP} <= set(oc.U)
    assert len(oc.ROWS) == oc.N == 64 and set(oc.LENGTHS) <= {len(r) for r in oc.ROWS}
    assert all(r == sorted(set(r)) and set(r) <= set(oc.U) for r in oc.ROWS)
    ka, kb, want = oc.named_pairs()
    assert np.array_equal(oc.expected(ka, kb), want)
    p, q, q1 = (oc.ROWS[oc.NAMES[n]] for n in ("edge_p", "edge_q", "edge_q1"))
    common = sorted(set(p) & set(q))
    assert [p.index(x) for x in common] == [63, 64, 127, 128] == [q.index(x) for x in common] and [q1.index(x) for x in common] == [62, 63, 126, 127]
    a, b = oc.ROWS[oc.NAMES["cross_a"]], oc.ROWS[oc.NAMES["cross_b"]]
    assert a[0] == b[-1] and oc.ROWS[oc.NAMES["first_a"]][0] == oc.ROWS[oc.NAMES["first_b"]][0] and oc.ROWS[oc.NAMES["last_a"]][-1] == oc.ROWS[oc.NAMES["last_b"]][-1]
    assert max(oc.ROWS[oc.NAMES["low"]]) < min(oc.ROWS[oc.NAMES["high"]])
    assert every[2][::oc.N + 1].tolist() == [len(r) for r in oc.ROWS]             # (k, k): the row's size


@pytest.mark.parametrize("threads", [1, 3])
def test_host_numpy_and_python_agree(every, threads):
    ka, kb, want = every
    rows = oc.rows_csr()
    got = indexio.rows_intersect_host(rows, None, ka, kb, threads=threads)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(indexio.rows_intersect_host(rows, rows, ka, kb, threads=threads), want)
    if threads == 1:
        assert np.array_equal(indexio.row_overlaps_from_rows(rows, None, ka, kb), want)
    # a second set: some rows in another order; slots are positions of the sets, not structure ids
    pick = [oc.NAMES[n] for n in ("third", "len0", "top", "edge_q", "len4200", "odds", "zero", "copy64")]
    rb = oc.rows_csr(pick)
    sa, sb = np.repeat(np.arange(oc.N, dtype=np.uint32), len(pick)), np.tile(np.arange(len(pick), dtype=np.uint32), oc.N)
    want_b = oc.expected(sa, np.array(pick, np.uint32)[sb])
    assert np.array_equal(indexio.rows_intersect_host(rows, rb, sa, sb, threads=threads), want_b)
    assert np.array_equal(indexio.row_overlaps_from_rows(rows, rb, sa, sb), want_b)
    # the order of the pairs is the order of the result: by work descending, ascending, and the same pair twice
    w = oc.work(ka, kb)
    for order in (np.argsort(-w, kind="stable"), np.argsort(w, kind="stable"), np.array([5, 5, 70, 5, 70])):
        assert np.array_equal(indexio.rows_intersect_host(rows, None, ka[order], kb[order], threads=threads), want[order])
    assert len(indexio.rows_intersect_host(rows, None, [], [])) == 0


def test_host_refusals():
    h, off = oc.rows_csr([1, 2, 3])
    L = _lib.load()
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)

    def call(hp, op, n, ka, kb, P):
        out = u32p()
        out.contents = C.c_uint32(7)                  # not NULL going in
        arr = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=np.uint32 if t is u32p else np.uint64).ctypes.data_as(t)
        rc = L.fdgpu_rows_intersect_host(arr(hp, u32p), arr(op, u64p), n, None, None, 0, arr(ka, u32p), arr(kb, u32p), P, 1, C.byref(out))
        return rc, bool(out)
    assert call(h, off, 3, [0, 3], [0, 0], 2) == (-1, False)                      # a slot at the row count
    assert call(h, off, 3, [0, 0], [0, 3], 2) == (-1, False)
    assert call(h, off, 3, None, [0], 1) == (-1, False) and call(h, off, 3, [0], None, 1) == (-1, False)      # a NULL array with a count
    assert call(h, off, 3, [0], [0], 1 << 32) == (-1, False)                      # refused before anything is read
    assert call(h, None, 3, [0], [0], 1) == (-1, False)
    assert call(h, off[::-1].copy(), 3, [0], [0], 1) == (-1, False)              # offsets that descend
    out = u32p()
    assert L.fdgpu_rows_intersect_host(None, np.zeros(1, np.uint64).ctypes.data_as(u64p), 0, None, None, 0, None, None, 0, 1, C.byref(out)) == 0 and bool(out)
    L.fdgpu_free(out)
    for ka, kb in (([3], [0]), ([0], [3]), ([-1], [0]), ([0, 1], [0]), ([0.5], [0])):
        with pytest.raises(ValueError, match="^rows intersect:"):
            indexio.rows_intersect_host((h, off), None, ka, kb)
        with pytest.raises((ValueError, IndexError)):
            indexio.row_overlaps_from_rows((h, off), None, ka, kb)


def test_jaccard_reaches_at_the_edges():
    r = indexio.jaccard_reaches
    assert r(9, 10, 0.9) is True and r(8999, 10000, 0.9) is False and r(9000, 10000, 0.9) is True      # inter * 10^4 == T * union exactly
    assert r(0, 0, 0.5) is False and r(0, 0, 1.0) is False and r(0, 0, 0.0001) is False                # union == 0 never reaches
    assert r(10, 10, 1.0) is True and r(9999, 10000, 1.0) is False and r((1 << 32) - 2, (1 << 32) - 1, 1.0) is False
    assert r(1, 10000, 0.0001) is True and r(1, 10001, 0.0001) is False and r(0, 5, 0.0001) is False
    assert r(2 ** 32 - 1, 2 ** 32 - 1, 1.0) is True                                                    # 64-bit: no wrap at 2^32 * 10^4
    assert indexio.jaccard_floor(0.9) == 9000 and indexio.jaccard_floor(1.0) == 10000 and indexio.jaccard_floor(0.0001) == 1
    got = r(np.array([9, 8, 0]), np.array([10, 10, 0]), 0.85)
    assert got.dtype == bool and got.tolist() == [True, False, False]
    for bad in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            r(1, 1, bad)


@pytest.mark.parametrize("first_id", oc.FIRST_IDS)
def test_row_overlaps_host_does_not_depend_on_pool_or_window(files, every, first_id):
    f = files[first_id]
    rows = indexio.rows_host(*f[:4], first_id=first_id)
    assert np.array_equal(rows[0], oc.rows_csr()[0]) and np.array_equal(rows[1], oc.rows_csr()[1])      # the index holds the prescribed rows
    ka, kb, want = oc.named_pairs()
    rng = np.random.Generator(np.random.PCG64(3))
    extra = rng.integers(0, oc.N * oc.N, size=150)
    ka, kb, want = np.concatenate([ka, every[0][extra]]), np.concatenate([kb, every[1][extra]]), np.concatenate([want, every[2][extra]])
    n_a, n_b = (np.array([len(oc.ROWS[k]) for k in x], np.uint32) for x in (ka, kb))
    distinct = len(np.unique(ka)) + len(np.unique(kb))
    for pool in POOLS:
        for window in WINDOWS:
            st = {}
            got = indexio.row_overlaps_host(f, None, first_id + ka.astype(np.int64), first_id + kb.astype(np.int64), window=window, pool_hashes=pool,
                                            threads=2, stats=st)
            assert all(g.dtype == np.uint32 for g in got)
            assert np.array_equal(got[0], want) and np.array_equal(got[1], n_a) and np.array_equal(got[2], n_b), (pool, window)
            assert st["distinct"] == distinct and st["extractions"] >= distinct and (pool < (1 << 40) or st["extractions"] == distinct)
            assert pool > 5000 or st["extractions"] > distinct                   # a small pool extracts rows again
    # two indices: the second holds the same rows at other ids
    g = files[5] if first_id == 0 else files[0]
    got = indexio.row_overlaps_host(f, g, first_id + ka.astype(np.int64), g[4] + kb.astype(np.int64), window=7, pool_hashes=9000)
    assert np.array_equal(got[0], want)
    empty = indexio.row_overlaps_host(f, None, [], [])
    assert all(len(x) == 0 and x.dtype == np.uint32 for x in empty)
    with pytest.raises(ValueError):
        indexio.row_overlaps_host(f, None, [first_id + oc.N], [first_id])
    with pytest.raises(ValueError):
        indexio.row_overlaps_host(f, None, [first_id - 1], [first_id])


def _overlap_tsv(tids_a, tids_b, ka, kb, floor=None):
    rows = []
    for a, b in zip(ka, kb):
        x, y = oc.SETS[int(a)], oc.SETS[int(b)]
        inter, union = len(x & y), len(x | y)
        if floor is not None and not (union > 0 and inter * 10000 >= round(floor * 10000) * union):
            continue
        rows.append("\t".join([str(a), tids_a[a], str(len(x)), str(b), tids_b[b], str(len(y)), str(inter), str(union), f"{inter / max(union, 1):.4f}"]) + "\n")
    return "".join(rows)


def test_overlap_host_command(tmp_path, no_device, capsys):
    one, two, out, pf = (str(tmp_path / n) for n in ("one", "two", "OUT.tsv", "pairs.txt"))
    tids = write_index(one)
    tids2 = write_index(two, tids=[f"u{k}" for k in range(oc.N)])
    ka, kb, _ = oc.named_pairs()
    ka, kb = ka.tolist() + [3, 3], kb.tolist() + [9, 9]                            # the same pair twice
    with open(pf, "w") as f:
        f.writelines(f"{tids[a]}\t{tids[b]}\n" for a, b in zip(ka, kb))
    capsys.readouterr()
    assert _status(["overlap", "--host", "-i", one, "--pairs", pf, "-o", out, "-t", "3", "--verify", "-v", "--pool-mb", "1", "--window", "5"]) == 0
    cap = capsys.readouterr()
    assert open(out).read() == _overlap_tsv(tids, tids, ka, kb)
    distinct = len(set(ka)) + len(set(kb))
    assert cap.out == f"[OK] {one}: {len(ka)} pairs, {distinct} distinct rows\n"
    assert f"row extractions for {distinct} distinct rows" in cap.err and "[INFO] overlap on the host" in cap.err
    # standard output, a floor, the second index
    with open(pf, "w") as f:
        f.writelines(f"{tids[a]}\t{tids2[b]}\n" for a, b in zip(ka, kb))
    assert _status(["overlap", "--host", "-i", one, "--against", two, "--pairs", pf, "--min-jaccard", "0.5"]) == 0
    cap = capsys.readouterr()
    want = _overlap_tsv(tids, tids2, ka, kb, floor=0.5)
    n_kept = want.count("\n")
    assert 0 < n_kept < len(ka) and cap.out == want + f"[OK] {one} x {two}: {len(ka)} pairs, {distinct} distinct rows, {n_kept} at or above 0.5\n"
    open(pf, "w").close()
    assert _status(["overlap", "--host", "-i", one, "--pairs", pf, "-o", out]) == 0               # no pair: an empty file
    assert open(out).read() == "" and "0 pairs" in capsys.readouterr().out
    assert not [f for f in os.listdir(tmp_path) if "overlap-tmp" in f]


def test_overlap_refusals_before_any_device_call(tmp_path, no_device, capsys):
    one, two, other, out, pf = (str(tmp_path / n) for n in ("one", "two", "other", "OUT.tsv", "pairs.txt"))
    tids = write_index(one)
    write_index(two, tids=[f"u{k}" for k in range(oc.N)])
    write_index(other, nbin_angle=5)
    twice = str(tmp_path / "twice")
    write_index(twice, tids=["t0", "t0"] + [f"t{k}" for k in range(2, oc.N)])
    for ext in ("", ".offset", ".lookup", ".type"):                           # a sharded prefix: no single index
        with open(str(tmp_path / "sh") + ".shard0of2" + ext, "wb") as f:
            f.write(open(one + ext, "rb").read())
    with open(pf, "w") as f:
        f.write("t1\tt2\nt3\tt4\n")
    names = sorted(os.listdir(tmp_path))
    capsys.readouterr()
    for x in ("0", "-0.5", "1.01", "nan"):
        assert _status(["overlap", "-i", one, "--pairs", pf, "-o", out, "--min-jaccard", x]) == 1
    assert _status(["overlap", "-i", one, "--pairs", pf, "-o", out, "--window", "0"]) == 1
    assert _status(["overlap", "-i", one, "--pairs", pf, "-o", out, "--pool-mb", "0"]) == 1
    capsys.readouterr()
    assert _status(["overlap", "-i", str(tmp_path / "sh"), "--pairs", pf, "-o", out]) == 1 and "sharded" in capsys.readouterr().out
    assert _status(["overlap", "-i", one, "--against", other, "--pairs", pf, "-o", out]) == 1 and ".type files differ" in capsys.readouterr().out
    assert _status(["overlap", "-i", str(tmp_path / "nope"), "--pairs", pf, "-o", out]) == 2
    assert _status(["overlap", "-i", one, "--pairs", str(tmp_path / "nope.txt"), "-o", out]) == 2
    capsys.readouterr()
    unknown = str(tmp_path / "unknown.txt")
    with open(unknown, "w") as f:
        f.writelines(f"x{k}\tt1\n" for k in range(12))
    names.append("unknown.txt")
    assert _status(["overlap", "-i", one, "--pairs", unknown, "-o", out]) == 1
    msg = capsys.readouterr().out
    assert "12 tid(s)" in msg and "x9" in msg and "x10" not in msg and "..." in msg
    assert _status(["overlap", "-i", one, "--against", two, "--pairs", pf, "-o", out]) == 1      # tid_b is looked up in the second index
    assert "t2" in capsys.readouterr().out
    with open(unknown, "w") as f:
        f.write("t0\tt5\n")
    assert _status(["overlap", "-i", twice, "--pairs", unknown, "-o", out]) == 1 and "more than one row" in capsys.readouterr().out
    with open(unknown, "w") as f:
        f.write("t1 t2\n")
    assert _status(["overlap", "-i", one, "--pairs", unknown, "-o", out]) == 1 and "tid_a<TAB>tid_b" in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path)) == sorted(names) and tids[1] == "t1"


def _reaches(ta, tb, where, floor):
    x, y = oc.SETS[where[ta]], oc.SETS[where[tb]]
    return len(x | y) > 0 and len(x & y) * 10000 >= round(floor * 10000) * len(x | y)


def test_dups_and_cluster_host_min_jaccard(tmp_path, no_device, capsys):
    one, conf, out, red, red_all = (str(tmp_path / n) for n in ("one", "confirm.tsv", "OUT.tsv", "red.txt", "red_all.txt"))
    tids = write_index(one)
    where = {t: k for k, t in enumerate(tids)}
    F = 0.9
    # dups: exactly the rows of --confirm whose integers reach F
    assert _status(["dups", "--host", "-i", one, "-o", conf, "--confirm", "--min-similarity", "0.3", "-t", "2"]) == 0
    capsys.readouterr()
    assert _status(["dups", "--host", "-i", one, "-o", out, "--min-jaccard", str(F), "--min-similarity", "0.3", "-t", "2", "--window", "9"]) == 0
    line = capsys.readouterr().out
    all_rows = open(conf).readlines()
    want = [l for l in all_rows if _reaches(l.split("\t")[1], l.split("\t")[4], where, F)]
    assert 0 < len(want) < len(all_rows) and open(out).readlines() == want
    n_ident = sum(l.split("\t")[9] == "identical" for l in want)
    assert f"{len(want)} pairs ({n_ident} identical)" in line
    for x in ("0", "1.5", "nan"):
        assert _status(["dups", "--host", "-i", one, "-o", out, "--min-jaccard", x]) == 1
    # cluster: the TSV of --confirm; --redundant lists the members that reach F, the others are kept
    assert _status(["cluster", "--host", "-i", one, "-o", conf, "--confirm", "--redundant", red_all, "--min-similarity", "0.5"]) == 0
    base_line = capsys.readouterr().out
    assert _status(["cluster", "--host", "-i", one, "-o", out, "--min-jaccard", str(F), "--redundant", red, "--min-similarity", "0.5"]) == 0
    line = capsys.readouterr().out
    assert open(out).read() == open(conf).read()
    members = [l.split("\t") for l in open(conf).readlines() if l.split("\t")[9] != "representative"]
    assert [m[4] for m in sorted(members, key=lambda m: int(m[3]))] == open(red_all).read().split()
    reach = sorted((int(m[3]), m[4]) for m in members if _reaches(m[1], m[4], where, F))
    assert 0 < len(reach) < len(members) and open(red).read().split() == [t for _, t in reach]
    assert line == base_line.rstrip("\n") + f", {len(members) - len(reach)} members below the exact floor kept\n"
    assert _status(["cluster", "--host", "-i", one, "-o", out, "--min-jaccard", "2"]) == 1
    # a member below the floor counts among the kept rows of the refusal: give it the tid of a member that is listed
    below = next(m for m in members if not _reaches(m[1], m[4], where, F))
    shared = list(tids)
    shared[int(below[3])] = reach[0][1]
    two = str(tmp_path / "two")
    write_index(two, tids=shared)
    capsys.readouterr()
    assert _status(["cluster", "--host", "-i", two, "-o", out, "--redundant", red, "--min-similarity", "0.5"]) == 0      # without the floor both are members
    assert _status(["cluster", "--host", "-i", two, "-o", out, "--min-jaccard", str(F), "--redundant", red, "--min-similarity", "0.5"]) == 1
    assert reach[0][1] in capsys.readouterr().out
