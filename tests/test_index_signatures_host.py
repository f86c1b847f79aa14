"""Index signatures on the host, no GPU: fdgpu_signatures_host (indexio.signatures_host) and indexio.signatures_from_rows against a pure-Python
statement of the definition on hand-made rows and against the reduction of the oracle's hashes, fdgpu_signature_pairs_host against a numpy
brute force on hand-made tables, and `python -m folddisco_amd dups --host` with its refusals, which come before any device call."""
import os

import numpy as np
import pytest

import oracle
from folddisco_amd import indexio
from tests import signature_cases as sc
from tests.helpers import packed_to_oracle_structs

PAIR_FIELDS = list(indexio.SIGNATURE_PAIR_DTYPE.names)


def _same(a, b):
    return a.dtype == b.dtype == indexio.SIGNATURE_DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()


def _raw(p):
    """the twelve-byte records of a pair result"""
    out = np.zeros(len(p), indexio.SIGNATURE_PAIR_DTYPE)
    for k in PAIR_FIELDS:
        out[k] = p[k]
    return out


@pytest.fixture(scope="module")
def want():
    """the expected table of the hand-made rows, once"""
    return sc.table_of(sc.ROWS, indexio.SIGNATURE_DTYPE)


@pytest.fixture(scope="module")
def hand_made():
    return {f: sc.index(f) for f in sc.FIRST_IDS}


def test_hand_made_rows_have_the_cases(want, hand_made):
    """the shape the cases rely on"""
    assert indexio.SIGNATURE_DTYPE.itemsize == 280 and indexio.SIGNATURE_PAIR_DTYPE.itemsize == 12
    n = want["n"]
    assert all(n[s] == 0 for s in sc.HOLES) and sc.HOLES == (0, 350, sc.N - 1)
    assert [int(n[s]) for s in (sc.ONE, sc.R63, sc.R64, sc.R65, sc.LONG)] == [1, 63, 64, 65, sc.N_LONG]
    assert (want["sk"][sc.ONE_BUCKET] != sc.EMPTY).tolist() == [b == 7 for b in range(64)] and n[sc.ONE_BUCKET] == 10
    assert (want["sk"][sc.ALL_BUCKETS] != sc.EMPTY).all()
    h1, h2 = sc.SWAPPED_PAIR
    assert h1 < h2 and sc.bucket(h1) == sc.bucket(h2) and sc.value(h2) < sc.value(h1) and want["sk"][sc.SWAPPED][sc.bucket(h1)] == sc.value(h2)
    assert want[sc.SAME_A].tobytes() == want[sc.SAME_B].tobytes() and n[sc.SAME_A] == 200
    assert n[sc.NEAR_B] == n[sc.NEAR_A] + 1 and want["d0"][sc.NEAR_A] != want["d0"][sc.NEAR_B] and (want["sk"][sc.NEAR_A] != want["sk"][sc.NEAR_B]).sum() <= 1
    empty = want[0]
    assert (empty["n"], empty["reserved"], empty["d0"], empty["d1"]) == (0, 0, 0, 0) and (empty["sk"] == sc.EMPTY).all()
    assert (want["reserved"] == 0).all() and sc.mix(0) == 0xE220A8397B1DCDAF          # splitmix64's first output for the seed 0
    for f, (v, h, o, lists) in hand_made.items():
        lens = np.diff(o.astype(np.int64)).tolist()
        assert set(sc.LIST_BYTES) <= set(lens) and int(o[-1]) == len(v)
        assert indexio.verify_host(v, h, o, sc.N, first_id=f).ok and [sc.decode(sc.encode(l)) for l in lists] == lists
        assert min(l[0] for l in lists) == f + 1 and max(l[-1] for l in lists) == f + sc.NEAR_B


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_signatures_host_equals_python(hand_made, want, first_id, threads):
    v, h, o, _ = hand_made[first_id]
    keep = [x.copy() for x in (v, h, o)]
    assert _same(indexio.signatures_host(v, h, o, sc.N, first_id=first_id, threads=threads), want)      # the default range
    for lo, hi in sc.RANGES:
        got = indexio.signatures_host(v, h, o, sc.N, first_id=first_id, lo=first_id + lo, hi=first_id + hi, threads=threads)
        assert _same(got, want[lo:hi]), (lo, hi)
    assert all(np.array_equal(x, y) for x, y in zip((v, h, o), keep))                                   # the source arrays are untouched


@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_signatures_from_rows_equals_python(hand_made, want, first_id):
    v, h, o, _ = hand_made[first_id]
    rows = indexio.rows_host(v, h, o, sc.N, first_id=first_id, threads=2)
    assert all(np.array_equal(x, y) for x, y in zip(rows, sc.rows_csr()))
    assert _same(indexio.signatures_from_rows(*rows), want)
    assert _same(indexio.signatures_from_rows(*sc.rows_csr(350, 612)), want[350:612])


def test_signatures_host_empty_index_and_errors():
    got = indexio.signatures_host(np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(1, np.uint64), 10, first_id=3)
    assert len(got) == 10 and (got["n"] == 0).all() and (got["sk"] == sc.EMPTY).all() and (got["d0"] == 0).all() and (got["d1"] == 0).all()
    from tests.rebase_cases import pack
    v, h, o = pack([[100, 105], [101, 300], [120]])
    assert indexio.signatures_host(v, h, o, 1000, first_id=100)["n"].sum() == 5
    for lo, hi in ((99, 200), (100, 1101), (200, 150)):                     # a range past the index, or backwards
        with pytest.raises(ValueError, match=r"\(-1\)"):
            indexio.signatures_host(v, h, o, 1000, first_id=100, lo=lo, hi=hi)
    with pytest.raises(ValueError, match=r"\(-1\)"):                        # an id outside [first_id, first_id + n): the refusal of the rows
        indexio.signatures_host(*pack([[100, 105], [101, 1100], [120]]), 1000, first_id=100, lo=100, hi=400)


def test_signatures_host_equals_the_reduction_of_the_oracles_hashes():
    """an oracle-built index over a dozen small structures: its signatures are the reduction of the per-structure lists it was built from"""
    from folddisco_amd import synth
    structs = packed_to_oracle_structs(synth.to_packed(synth.generate(12, seed=31)))
    h, off = oracle.hash_batch(structs)
    ix = oracle.build_index_from_lists(h, off)
    src = (ix.values().copy(), ix.hashes().copy(), ix.offsets().copy())
    off = np.asarray(off).astype(np.int64)
    want = sc.table_of([np.asarray(h[off[s]:off[s + 1]]).tolist() for s in range(12)], indexio.SIGNATURE_DTYPE)
    assert want["n"].sum() > 1000
    assert _same(indexio.signatures_host(*src, 12, threads=2), want)
    assert _same(indexio.signatures_host(*src, 12, lo=3, hi=9), want[3:9])
    assert _same(indexio.signatures_from_rows(np.asarray(h, np.uint32), off), want)


# ---- pairs
@pytest.fixture(scope="module")
def tables():
    return {n: sc.pair_table(n, 100 + n, indexio.SIGNATURE_DTYPE) for n in sc.PAIR_SIZES}


def test_pair_tables_have_the_cases(tables):
    A = tables[129]
    on = sc.brute_pairs(A[:6], None, 48, indexio.SIGNATURE_PAIR_DTYPE)
    rec = {(int(r["a"]), int(r["b"])): (int(r["match"]), int(r["filled"])) for r in on}
    assert rec[(0, 1)] == (48, 64) and (0, 2) not in rec and rec[(3, 4)] == (24, 32) and (3, 5) not in rec      # on the threshold; one match below it
    low = {(int(r["a"]), int(r["b"])): (int(r["match"]), int(r["filled"])) for r in sc.brute_pairs(A[:6], None, 47, indexio.SIGNATURE_PAIR_DTYPE)}
    assert low[(0, 2)] == (47, 64) and (3, 5) not in low and 23 * 64 < 47 * 32
    assert A["n"][6] == 0 and A["n"][7] == 0 and (A["sk"][7] == A["sk"][0]).all()
    every = sc.brute_pairs(A, None, 1, indexio.SIGNATURE_PAIR_DTYPE)
    assert len(every) > 1000 and not np.isin(every["a"], (6, 7)).any() and not np.isin(every["b"], (6, 7)).any()      # empty signatures are never reported
    assert (every["filled"] < 64).any() and (every["filled"] == 64).any()
    full = {(int(r["a"]), int(r["b"])): int(r["flags"]) for r in sc.brute_pairs(A[:10], None, 64, indexio.SIGNATURE_PAIR_DTYPE)}
    assert full[(0, 8)] == 1 and full[(0, 9)] == 0 and full[(8, 9)] == 0


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("n", sc.PAIR_SIZES)
def test_signature_pairs_host_equals_brute_force(tables, n, threads):
    A = tables[n]
    for B in (None, sc.other_table(A, 7)):
        for thr in sc.THRESHOLDS:
            want = sc.brute_pairs(A, B, thr, indexio.SIGNATURE_PAIR_DTYPE)
            got = indexio.signature_pairs_host(A, B, thr64=thr, threads=threads)
            assert got.dtype == indexio.SIGNATURE_PAIRS_DTYPE and np.array_equal(_raw(got), want), (n, B is None, thr)
            assert np.array_equal(got["estimate"], want["match"] / np.maximum(want["filled"], 1))
            if B is not None:
                assert len(want) > 0 and (want["flags"] & 1).any()      # the copies of A's records


def test_signature_pairs_host_threshold_cap_and_refusals(tables):
    A = tables[129]
    assert np.array_equal(indexio.signature_pairs_host(A, min_similarity=0.75), indexio.signature_pairs_host(A, thr64=48))
    assert [indexio.signature_threshold(x) for x in (0.9, 0.75, 1.0, 0.001, 0.0, 2.0)] == [58, 48, 64, 1, 1, 64]
    for B in (None, sc.other_table(A, 7)):
        true = len(sc.brute_pairs(A, B, 1, indexio.SIGNATURE_PAIR_DTYPE))
        assert len(indexio.signature_pairs_host(A, B, thr64=1, max_pairs=true)) == true      # the cap itself fits
        with pytest.raises(indexio.SignaturePairsOverflow, match=r"\(-4\)") as e:
            indexio.signature_pairs_host(A, B, thr64=1, max_pairs=true - 1, threads=2)
        assert e.value.count == true
    for thr in (0, 65):
        with pytest.raises(ValueError, match=r"\(-1\)"):
            indexio.signature_pairs_host(A, thr64=thr)
    assert len(indexio.signature_pairs_host(A[:0], thr64=1)) == 0 and len(indexio.signature_pairs_host(A, A[:0], thr64=1)) == 0


# ---- the command
N = 40
COPIES = (3, 17, 30)            # structures of the first index that the second one holds too, under other tids


@pytest.fixture(scope="module")
def lists():
    """sorted unique hashes of every structure of a small synthetic batch as CSR: the oracle's, no product code"""
    from folddisco_amd import synth
    h, off = oracle.hash_batch(packed_to_oracle_structs(synth.to_packed(synth.generate(N, seed=31))))
    return np.asarray(h, np.uint32), np.asarray(off, np.uint64)


def _take(lists, ids):
    h, off = lists
    out = np.zeros(len(ids) + 1, np.uint64)
    out[1:] = np.cumsum([int(off[k + 1] - off[k]) for k in ids])
    return np.concatenate([h[int(off[k]):int(off[k + 1])] for k in ids]), out


def _write_index(prefix, lists, tids, **type_kw):
    h, off = lists
    ix = oracle.build_index_from_lists(h, off)
    n = len(off) - 1
    indexio.write_index_files(prefix, ix.values().copy(), ix.hashes().copy(), ix.offsets().copy())
    indexio.save_lookup_py(prefix + ".lookup", tids, 50 + np.arange(n, dtype=np.uint64), np.full(n, 80.5, np.float32))
    indexio.save_type(prefix + ".type", n, **type_kw)


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


def _second(lists):
    """the second index: the COPIES of the first, then one structure less one hash, then two others twice"""
    h, off = lists
    near = h[int(off[5]):int(off[6])][:-1]
    parts = [h[int(off[k]):int(off[k + 1])] for k in COPIES] + [near] + [h[int(off[k]):int(off[k + 1])] for k in (8, 8)]
    out = np.zeros(len(parts) + 1, np.uint64)
    out[1:] = np.cumsum([len(p) for p in parts])
    return np.concatenate(parts), out


def _jaccard(x, y):
    x, y = set(x.tolist()), set(y.tolist())
    return len(x & y) / len(x | y)


def _expected_tsv(la, ta, lb, tb, thr64, identical_only=False, confirm=False):
    """the command's rows from the Python forms alone: signatures_from_rows, the numpy brute force, a set Jaccard"""
    A = indexio.signatures_from_rows(*la)
    B = None if lb is None else indexio.signatures_from_rows(*lb)
    rows = []
    for r in sc.brute_pairs(A, B, thr64, indexio.SIGNATURE_PAIR_DTYPE):
        a, b, ident = int(r["a"]), int(r["b"]), bool(r["flags"] & 1)
        if identical_only and not ident:
            continue
        lb_, tb_, B_ = (la, ta, A) if lb is None else (lb, tb, B)
        cols = [str(a), ta[a], str(int(A["n"][a])), str(b), tb_[b], str(int(B_["n"][b])), str(int(r["match"])), str(int(r["filled"])),
                f"{int(r['match']) / int(r['filled']):.4f}", "identical" if ident else "similar"]
        if confirm:
            cols.append(f"{_jaccard(la[0][int(la[1][a]):int(la[1][a + 1])], lb_[0][int(lb_[1][b]):int(lb_[1][b + 1])]):.4f}")
        rows.append("\t".join(cols) + "\n")
    return "".join(rows)


def test_dups_host_command(tmp_path, lists, no_device, capsys):
    one, two, out = str(tmp_path / "one"), str(tmp_path / "two"), str(tmp_path / "OUT.tsv")
    ta, tb = [f"s{k}" for k in range(N)], [f"m{k}" for k in range(6)]
    lb = _second(lists)
    _write_index(one, lists, ta)
    _write_index(two, lb, tb)
    # --against: the drop against the database
    assert _status(["dups", "--host", "-i", two, "--against", one, "-o", out, "-t", "3", "--verify", "-v", "--min-similarity", "0.5"]) == 0
    cap = capsys.readouterr()
    text = open(out).read()
    assert text == _expected_tsv(lb, tb, lists, ta, 32)
    got = [l.split("\t") for l in text.splitlines()]
    ident = [(int(c[0]), int(c[3])) for c in got if c[9] == "identical"]
    assert ident == [(0, 3), (1, 17), (2, 30), (4, 8), (5, 8)] and ("3", "5") in [(c[0], c[3]) for c in got if c[9] == "similar"]
    assert cap.out == f"[OK] {two} x {one}: 6 x {N} structures, {len(got)} pairs (5 identical), threshold 32/64\n" and "[INFO] dups on the host" in cap.err
    # inside one index, on standard output, the default threshold
    assert _status(["dups", "--host", "-i", two]) == 0
    cap = capsys.readouterr()
    want = _expected_tsv(lb, tb, None, None, 58)
    assert cap.out == want + f"[OK] {two}: 6 structures, {len(want.splitlines())} pairs (1 identical), threshold 58/64\n"
    assert "4\tm4\t" in want and "\t5\tm5\t" in want
    # --identical-only and --confirm
    assert _status(["dups", "--host", "-i", two, "--against", one, "-o", out, "--identical-only", "--confirm", "--window", "7"]) == 0
    text = open(out).read()
    assert text == _expected_tsv(lb, tb, lists, ta, 64, identical_only=True, confirm=True) and len(text.splitlines()) == 5
    assert all(l.split("\t")[9:] == ["identical", "1.0000"] for l in text.splitlines())
    assert capsys.readouterr().out.endswith("5 pairs (5 identical), threshold 64/64\n")
    assert _status(["dups", "--host", "-i", two, "--against", one, "-o", out, "--confirm", "--min-similarity", "0.5", "-t", "2"]) == 0
    text = open(out).read()
    assert text == _expected_tsv(lb, tb, lists, ta, 32, confirm=True)
    near = [l.split("\t") for l in text.splitlines() if l.split("\t")[:4:3] == ["3", "5"]]
    n5 = int(lists[1][6] - lists[1][5])
    assert len(near) == 1 and near[0][9] == "similar" and near[0][10] == f"{(n5 - 1) / n5:.4f}"
    capsys.readouterr()
    # more pairs than --max-pairs: the true count, no file
    os.remove(out)
    assert _status(["dups", "--host", "-i", two, "--against", one, "-o", out, "--min-similarity", "0.5", "--max-pairs", "3"]) == 1
    assert f"{len(got)} pairs" in capsys.readouterr().out and not os.path.exists(out)
    assert not [f for f in os.listdir(tmp_path) if "dups-tmp" in f]


def test_dups_refusals_before_any_device_call(tmp_path, lists, no_device, capsys):
    one, two, out = str(tmp_path / "one"), str(tmp_path / "two"), str(tmp_path / "OUT.tsv")
    _write_index(one, lists, [f"s{k}" for k in range(N)])
    _write_index(two, _second(lists), [f"m{k}" for k in range(6)])
    other = str(tmp_path / "other")
    _write_index(other, _second(lists), [f"m{k}" for k in range(6)], nbin_dist=8)
    bad = str(tmp_path / "bad")
    _write_index(bad, lists, [f"s{k}" for k in range(N)])
    with open(bad, "ab") as f:
        f.write(b"\x01")                                                                              # what check_index_files finds
    for ext in ("", ".offset", ".lookup", ".type"):                                                   # a sharded prefix: no single index
        with open(str(tmp_path / "sh") + ".shard0of2" + ext, "wb") as f:
            f.write(open(two + ext, "rb").read())
    names = sorted(os.listdir(tmp_path))
    capsys.readouterr()
    assert _status(["dups", "-i", bad, "-o", out]) == 1 and "inconsistent" in capsys.readouterr().out
    assert _status(["dups", "-i", one, "--against", bad, "-o", out]) == 1 and "inconsistent" in capsys.readouterr().out
    for x in ("0", "-0.5", "1.01", "nan"):
        assert _status(["dups", "-i", one, "-o", out, "--min-similarity", x]) == 1                    # outside (0, 1]
    assert _status(["dups", "-i", one, "--against", one, "-o", out]) == 1                             # --against equal to -i
    assert _status(["dups", "-i", one, "--against", str(tmp_path / "." / "one"), "-o", out]) == 1
    capsys.readouterr()
    assert _status(["dups", "-i", one, "--against", other, "-o", out]) == 1                           # non-joinable .type
    assert "num_bin_dist" in capsys.readouterr().out
    assert _status(["dups", "-i", str(tmp_path / "sh"), "-o", out]) == 1 and "sharded" in capsys.readouterr().out
    assert _status(["dups", "-i", one, "--against", str(tmp_path / "sh"), "-o", out]) == 1
    assert _status(["dups", "-i", str(tmp_path / "nope"), "-o", out]) == 2                            # missing files
    assert _status(["dups", "-i", one, "--against", str(tmp_path / "nope"), "-o", out]) == 2
    assert sorted(os.listdir(tmp_path)) == names
