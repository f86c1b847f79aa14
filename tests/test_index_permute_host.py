"""Index reorder on the host, no GPU: fdgpu_permute_host (indexio.permute_host) against hand-made lists permuted in Python and against the
oracle's builds in two orders, the ordering rules and lookup rows of `python -m folddisco_amd reorder`, its refusals, which come before any device
call, and the whole command with --host."""
import os

import numpy as np
import pytest

import oracle
from folddisco_amd import indexio
from tests import permute_cases as pc
from tests.helpers import packed_to_oracle_structs

PERMS = pc.permutations()


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


@pytest.fixture(scope="module")
def hand_made():
    return {f: pc.lists_of(f) for f in pc.FIRST_IDS}


def test_hand_made_index_has_the_edges(hand_made):
    """the shape the cases rely on: every id count, every byte length on both sides of the kernel's class boundaries, a list of all ids, and a
    last list of one byte that ends on the last value byte"""
    for f in pc.FIRST_IDS:
        lists = hand_made[f]
        v, h, o = pc.pack(lists)
        lens = np.diff(o.astype(np.int64)).tolist()
        assert set(pc.ID_COUNTS) <= {len(l) for l in lists} and set(pc.BYTE_LENGTHS) <= set(lens) and pc.N in {len(l) for l in lists}
        assert {pc.SORT_BYTES - 1, pc.SORT_BYTES, pc.SORT_BYTES + 1, pc.SORT_BYTES_LOW - 1, pc.SORT_BYTES_LOW, pc.SORT_BYTES_LOW + 1} <= set(lens)
        assert int(o[-1]) == len(v) and pc.LDS_BITS_LOW < pc.N
        assert indexio.verify_host(v, h, o, pc.N, first_id=f).ok
        assert [pc.decode(pc.encode(l)) for l in lists] == lists
        deltas = np.concatenate([np.diff(l) for l in lists if len(l) > 1])
        assert (deltas < 128).any() and (deltas >= 128).any()                # one-byte and two-byte deltas
    assert int(np.diff(pc.pack(hand_made[0])[2].astype(np.int64))[-1]) == 1  # the last list is one byte long
    assert min(l[0] for l in hand_made[2097000]) < (1 << 21) <= max(l[-1] for l in hand_made[2097000])


def test_permutations_are_permutations():
    assert sorted(PERMS) == ["evens_then_odds", "identity", "random", "reversal", "rotate1", "swap127_128"]
    for name, p in PERMS.items():
        assert np.array_equal(np.sort(p), np.arange(pc.N)), name
        assert np.array_equal(p[pc.inverse(p)], np.arange(pc.N)), name
    assert PERMS["evens_then_odds"][:4].tolist() == [0, pc.N // 2, 1, pc.N // 2 + 1] and PERMS["rotate1"][-1] == 0


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("name", sorted(PERMS))
@pytest.mark.parametrize("first_id", pc.FIRST_IDS)
def test_permute_host_equals_python(hand_made, first_id, name, threads):
    p = PERMS[name]
    _, src, want = pc.case(first_id, name)
    keep = [x.copy() for x in src]
    got = indexio.permute_host(*src, p, first_id=first_id, threads=threads)
    assert _eq(got, want)
    assert _eq(src, keep)                                                  # the source arrays are untouched
    assert indexio.verify_host(*got, n_structures=pc.N, first_id=first_id).ok
    assert _eq(indexio.permute_host(*got, pc.inverse(p), first_id=first_id, threads=threads), src)      # and back again
    if name == "identity":
        assert _eq(got, src)


def test_permute_host_empty_index():
    v, h, o = indexio.permute_host(np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.array([2, 0, 1], np.uint32))
    assert len(v) == 0 and len(h) == 0 and o.tolist() == [0]
    v, h, o = indexio.permute_host(np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert len(v) == 0 and len(h) == 0 and o.tolist() == [0]


def test_permute_host_errors():
    src = pc.pack([[100, 105], [101, 109], [109]])
    ident = np.arange(10, dtype=np.uint32)
    with pytest.raises(ValueError, match=r"\(-1\)"):                       # a wrong length: the index holds ids past first_id + 9
        indexio.permute_host(*src, ident[:9], first_id=100)
    with pytest.raises(ValueError, match=r"\(-1\)"):                       # a repeated value
        indexio.permute_host(*src, np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 8], np.uint32), first_id=100)
    with pytest.raises(ValueError, match=r"\(-1\)"):                       # a value >= n
        indexio.permute_host(*src, np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 10], np.uint32), first_id=100)
    with pytest.raises(ValueError, match=r"\(-1\)"):                       # an id below first_id
        indexio.permute_host(*src, ident, first_id=101)
    v, h, o = src
    bad = o.copy()
    bad[1], bad[2] = o[2], o[1]                                            # offsets that do not ascend
    with pytest.raises(ValueError, match=r"\(-1\)"):
        indexio.permute_host(v, h, bad, ident, first_id=100)
    bad = o.copy()
    bad[-1] += 1                                                           # the last list leaves the value bytes
    with pytest.raises(ValueError, match=r"\(-1\)"):
        indexio.permute_host(v, h, bad, ident, first_id=100)
    with pytest.raises(ValueError, match=r"\(-1\)"):                       # a varint without an end inside its list
        indexio.permute_host(np.array([0x80, 0x80, 0x80], np.uint8), np.array([1], np.uint32), np.array([0, 3], np.uint64), ident)
    with pytest.raises(ValueError, match=r"\(-1\)"):                       # six bytes
        indexio.permute_host(np.array([0x80] * 5 + [0], np.uint8), np.array([1], np.uint32), np.array([0, 6], np.uint64), ident)
    rev = ident[::-1].copy()
    assert _eq(indexio.permute_host(*src, rev, first_id=100), pc.pack([[104, 109], [100, 108], [100]]))      # the good call still passes


# ---- against the oracle: one batch built in two orders
N_ORACLE = 60


@pytest.fixture(scope="module")
def lists60():
    """sorted unique hashes of every structure of a small synthetic batch as CSR: the oracle's, no product code"""
    from folddisco_amd import synth
    return oracle.hash_batch(packed_to_oracle_structs(synth.to_packed(synth.generate(N_ORACLE, seed=31))))


def _oracle_index(lists, seq):
    """the oracle's index over the batch's structures taken in the order seq (position k of the index = structure seq[k]), ids from 0"""
    h, off = lists
    off = off.astype(np.int64)
    hh = np.concatenate([h[off[s]:off[s + 1]] for s in seq]) if len(seq) else h[:0]
    oo = np.concatenate([[0], np.cumsum([off[s + 1] - off[s] for s in seq])]).astype(np.uint64)
    ix = oracle.build_index_from_lists(hh, oo)
    return ix.values().copy(), ix.hashes().copy(), ix.offsets().copy()


@pytest.mark.parametrize("kind", ["reversal", "random", "rotate1"])
def test_permute_host_equals_oracle_build_in_the_new_order(lists60, kind):
    n = N_ORACLE
    k = np.arange(n)
    p = {"reversal": n - 1 - k, "random": np.random.Generator(np.random.PCG64(5)).permutation(n), "rotate1": (k + 1) % n}[kind].astype(np.uint32)
    first = _oracle_index(lists60, list(range(n)))
    second = _oracle_index(lists60, [int(s) for s in pc.inverse(p)])       # position j holds the structure k with p[k] = j
    got = indexio.permute_host(*first, p, threads=2)
    assert _eq(got, second)
    assert indexio.verify_host(*got, n_structures=n).ok


# ---- the ordering rules and the lookup rows
def _rows(tids, nres, plddt, db_keys=None):
    return indexio.lookup_rows(0, tids, nres, plddt, db_keys=db_keys)


def _apply(rows, new_id):
    """tids in their new order"""
    return [r.split("\t")[1] for r in indexio.permute_lookup_rows(rows, new_id, keep_db_keys=False)]


def test_order_from_lookup_by_column():
    rows = _rows(["b", "a10", "a9", "c", "a9x"], [30, 100, 9, 30, 9], [70.5, 9.0, 100.0, 70.5, 80.25])
    assert _apply(rows, indexio.order_from_lookup(rows, by="tid")) == ["a10", "a9", "a9x", "b", "c"]             # byte strings: "a10" < "a9"
    assert _apply(rows, indexio.order_from_lookup(rows, by="tid", descending=True)) == ["c", "b", "a9x", "a9", "a10"]
    assert _apply(rows, indexio.order_from_lookup(rows, by="nres")) == ["a9", "a9x", "b", "c", "a10"]            # numeric: 9 < 30 < 100; ties as they were
    assert _apply(rows, indexio.order_from_lookup(rows, by="nres", descending=True)) == ["a10", "b", "c", "a9", "a9x"]      # ... also when descending
    assert _apply(rows, indexio.order_from_lookup(rows, by="plddt")) == ["a10", "b", "c", "a9x", "a9"]           # numeric: 9 < 70.5 < 80.25 < 100
    assert _apply(rows, indexio.order_from_lookup(rows, by="plddt", descending=True)) == ["a9", "a9x", "b", "c", "a10"]
    p = indexio.order_from_lookup(rows, by="nres")
    assert p.dtype == np.uint32 and p.tolist() == [2, 4, 0, 3, 1]                                                 # new_id[k] = new position of row k
    with pytest.raises(ValueError, match="unknown sort key"):
        indexio.order_from_lookup(rows, by="size")
    with pytest.raises(ValueError, match="exactly one"):
        indexio.order_from_lookup(rows)
    with pytest.raises(ValueError, match="exactly one"):
        indexio.order_from_lookup(rows, by="tid", order_tids=["a"])


def test_order_from_lookup_by_tid_list():
    rows = _rows(["x", "y", "z"], [1, 2, 3], [1.0, 2.0, 3.0])
    assert indexio.order_from_lookup(rows, order_tids=["z", "x", "y"]).tolist() == [1, 2, 0]
    assert _apply(rows, indexio.order_from_lookup(rows, order_tids=["z", "x", "y"])) == ["z", "x", "y"]
    with pytest.raises(ValueError, match="'y' is missing"):
        indexio.order_from_lookup(rows, order_tids=["z", "x"])
    with pytest.raises(ValueError, match="'x' twice"):
        indexio.order_from_lookup(rows, order_tids=["z", "x", "x"])
    with pytest.raises(ValueError, match="'x' twice"):
        indexio.order_from_lookup(rows, order_tids=["z", "x", "y", "x"])
    with pytest.raises(ValueError, match="'w'.*does not hold"):
        indexio.order_from_lookup(rows, order_tids=["z", "x", "w"])
    dup = _rows(["x", "y", "x"], [1, 2, 3], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="appears twice"):
        indexio.order_from_lookup(dup, order_tids=["x", "y", "x"])
    assert _apply(dup, indexio.order_from_lookup(dup, by="tid")) == ["x", "x", "y"]                               # --by does not mind


def test_permute_lookup_rows_file_built():
    rows = _rows(["x", "y", "z"], [10, 20, 30], [80.5, 0.0, 91.25])
    out = indexio.permute_lookup_rows(rows, [2, 0, 1], keep_db_keys=False)
    assert "".join(out) == "".join(_rows(["y", "z", "x"], [20, 30, 10], [0.0, 91.25, 80.5]))                      # what `index` writes in the new order
    with pytest.raises(ValueError):
        indexio.permute_lookup_rows(rows, [0, 1], keep_db_keys=False)
    with pytest.raises(ValueError):
        indexio.permute_lookup_rows(rows, [0, 1, 1], keep_db_keys=False)


def test_permute_lookup_rows_foldcomp_built():
    rows = _rows(["x", "y", "z"], [10, 20, 30], [80.5, 0.0, 91.25], db_keys=[17, 4, 900])
    out = [r.rstrip("\n").split("\t") for r in indexio.permute_lookup_rows(rows, [2, 0, 1], keep_db_keys=True)]
    assert [r[0] for r in out] == ["0", "1", "2"] and [r[4] for r in out] == ["4", "900", "17"]                    # db_key travels with its row
    assert [r[1:4] for r in out] == [rows[k].rstrip("\n").split("\t")[1:4] for k in (1, 2, 0)]


# ---- the command
N = 40


@pytest.fixture(scope="module")
def lists40():
    from folddisco_amd import synth
    return oracle.hash_batch(packed_to_oracle_structs(synth.to_packed(synth.generate(N, seed=31))))


NRES = (50 + (np.arange(N) * 7) % 13).astype(np.uint64)                    # with ties
PLDDT = (60 + (np.arange(N) * 11) % 17).astype(np.float32)


def _write_index(prefix, lists, seq, **type_kw):
    """the index `index` would write over the batch's structures taken in the order seq; structure s has tid s<s>"""
    indexio.write_index_files(prefix, *_oracle_index(lists, seq))
    indexio.save_lookup_py(prefix + ".lookup", [f"s{s:02d}" for s in seq], NRES[seq], PLDDT[seq])
    indexio.save_type(prefix + ".type", len(seq), **type_kw)


@pytest.fixture
def no_device(monkeypatch):
    import folddisco_amd as fd

    def boom(*a, **k):
        raise AssertionError("a device was touched by a host-side reorder or before its validation ended")
    monkeypatch.setattr(fd, "Context", boom)


def _status(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


def _same_files(a, b):
    for ext in ("", ".offset", ".lookup", ".type"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext


def test_reorder_host_end_to_end(tmp_path, lists40, no_device, capsys):
    src, out = str(tmp_path / "ix"), str(tmp_path / "OUT")
    _write_index(src, lists40, list(range(N)))
    seq = [int(s) for s in np.random.Generator(np.random.PCG64(9)).permutation(N)]
    want = str(tmp_path / "want")
    _write_index(want, lists40, seq)
    order = str(tmp_path / "order.txt")
    with open(order, "w") as f:
        f.write("".join(f"s{s:02d}\n" for s in seq))
    assert _status(["reorder", "--host", "-i", src, "--order", order, "-o", out, "-t", "3", "--verify", "-v"]) == 0
    cap = capsys.readouterr()
    whole = indexio.read_index_files(want)
    moved = sum(1 for k, s in enumerate(seq) if k != s)
    assert cap.out.startswith(f"[OK] {out}: {N} structures reordered ({moved} moved), lists / postings / bytes: {len(whole[1])} / ")
    assert cap.out.strip().endswith(f" / {len(whole[0])}") and len(cap.out.strip().splitlines()) == 1
    assert "host" in cap.err and f"-> {len(whole[0])}" in cap.err
    _same_files(out, want)
    assert not [f for f in os.listdir(tmp_path) if "reorder-tmp" in f]
    # --by: descending tids are the reversal; ties of nres keep their old order
    rev = str(tmp_path / "rev")
    _write_index(rev, lists40, list(range(N))[::-1])
    assert _status(["reorder", "--host", "-i", src, "--by", "tid", "--desc", "-o", out]) == 0      # over an existing output, without --verify
    _same_files(out, rev)
    by_nres = str(tmp_path / "by_nres")
    _write_index(by_nres, lists40, sorted(range(N), key=lambda s: int(NRES[s])))
    assert _status(["reorder", "--host", "-i", src, "--by", "nres", "-o", out]) == 0
    _same_files(out, by_nres)
    # in place, and back with the inverse order
    keep = {ext: open(src + ext, "rb").read() for ext in ("", ".offset", ".lookup", ".type")}
    assert _status(["reorder", "--host", "-i", src, "--order", order]) == 0
    _same_files(src, want)
    assert _status(["reorder", "--host", "-i", src, "--by", "tid"]) == 0
    assert {ext: open(src + ext, "rb").read() for ext in keep} == keep
    assert not [f for f in os.listdir(tmp_path) if "reorder-tmp" in f]
    capsys.readouterr()


def test_reorder_refusals_before_any_device_call(tmp_path, lists40, no_device, capsys):
    src = str(tmp_path / "ix")
    _write_index(src, lists40, list(range(N)))
    tids = [f"s{s:02d}" for s in range(N)]

    def order_file(name, lines):
        p = str(tmp_path / name)
        with open(p, "w") as f:
            f.write("".join(t + "\n" for t in lines))
        return p
    good, missing = order_file("good.txt", tids[::-1]), order_file("missing.txt", tids[1:])
    twice, unknown = order_file("twice.txt", tids[:-1] + tids[:1]), order_file("unknown.txt", tids[:-1] + ["nope"])
    names = sorted(os.listdir(tmp_path))
    out = str(tmp_path / "OUT")
    assert _status(["reorder", "-i", src, "-o", out]) == 1                                   # neither --by nor --order
    assert _status(["reorder", "-i", src, "--by", "tid", "--order", good, "-o", out]) == 1   # both
    assert _status(["reorder", "-i", src, "--by", "size", "-o", out]) == 1                   # an unknown key
    capsys.readouterr()
    for f, word in ((missing, "missing"), (twice, "twice"), (unknown, "does not hold")):
        assert _status(["reorder", "-i", src, "--order", f, "-o", out]) == 1
        assert word in capsys.readouterr().out
    assert _status(["reorder", "-i", src, "--order", str(tmp_path / "none.txt"), "-o", out]) == 2      # a missing order file
    assert _status(["reorder", "-i", str(tmp_path / "nope"), "--by", "tid", "-o", out]) == 2           # a missing prefix
    assert sorted(os.listdir(tmp_path)) == names
    dup = str(tmp_path / "dup")
    _write_index(dup, lists40, list(range(N)))
    indexio.save_lookup_py(dup + ".lookup", ["s00"] + tids[:-1], NRES, PLDDT)                # .lookup itself holds a tid twice
    assert _status(["reorder", "-i", dup, "--order", good, "-o", out]) == 1
    assert "appears twice" in capsys.readouterr().out
    bad = str(tmp_path / "bad")
    _write_index(bad, lists40, list(range(N)))
    with open(bad, "ab") as f:
        f.write(b"\x01")                                                                     # what check_index_files finds
    assert _status(["reorder", "-i", bad, "--by", "tid", "-o", out]) == 1
    assert "inconsistent" in capsys.readouterr().out
    assert not [f for f in os.listdir(tmp_path) if f.startswith("OUT") or "reorder-tmp" in f]
