"""Index rows on the host, no GPU: fdgpu_rows_host (indexio.rows_host) against a pure-Python transposition of hand-made lists and against the
per-structure hash lists the oracle builds its index from, its refusals, and `python -m folddisco_amd rows --host` / the refusals of
`verify --structures`, which come before any device call."""
import os

import numpy as np
import pytest

import oracle
from folddisco_amd import indexio
from tests import rows_cases as rw
from tests.helpers import packed_to_oracle_structs


def _eq(a, b):
    return len(a) == len(b) == 2 and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def _cut(rows, lo, hi):
    """rows lo .. hi - 1 of a CSR pair"""
    h, off = rows
    return h[int(off[lo]):int(off[hi])], off[lo:hi + 1] - off[lo]


@pytest.fixture(scope="module")
def hand_made():
    out = {}
    for f in rw.FIRST_IDS:
        lists = rw.lists(f)
        out[f] = (lists, rw.pack(lists))
    return out


@pytest.fixture(scope="module")
def whole(hand_made):
    """the Python transposition of the whole index, once per first_id"""
    return {f: rw.expected_rows(lists, src[1], f, f + rw.N) for f, (lists, src) in hand_made.items()}


def test_hand_made_index_has_the_edges(hand_made):
    """the shape the cases rely on"""
    lists, (v, h, o) = hand_made[0]
    lens = np.diff(o.astype(np.int64)).tolist()
    assert set(rw.LENGTHS) <= set(lens) and max(lens) > 4096 and int(o[-1]) == len(v) and lens[-1] == 1      # the last list: one byte, on the last value byte
    assert indexio.verify_host(v, h, o, rw.N).ok and [rw.decode(rw.encode(l)) for l in lists] == lists
    assert min(l[0] for l in lists) == 0 and max(l[-1] for l in lists) == rw.N - 1
    blob = [rw.encode(l) for l in lists]
    assert any(len(b) > 257 and b[255] & 0x80 and not b[256] & 0x80 for b in blob)                            # a varint across the first step edge
    assert any(len(b) > 513 and b[510] & 0x80 and b[511] & 0x80 and not b[512] & 0x80 for b in blob)          # a three-byte one across the second
    assert sum(l == rw.DENSE for l in lists) == rw.N_DENSE and len(rw.DENSE) == 300
    used = set().union(*map(set, lists))
    assert not used & set(rw.HOLES) and not any(rw.EMPTY[0] <= x < rw.EMPTY[1] for x in used)
    assert rw.WINDOWS[3][0] == rw.HOLES[0] and rw.WINDOWS[3][0] < rw.HOLES[1] < rw.WINDOWS[3][1] - 1 and rw.WINDOWS[4][1] - 1 == rw.HOLES[2]
    assert sorted({hi - lo for lo, hi in rw.WINDOWS}) == [0, 1, 2, 256, 257, 500, 65536, 65537, (1 << 24) + 1]
    for lo, hi in rw.EDGE_WINDOWS:                   # lists wholly below, wholly above, and across either edge
        assert any(l[-1] < lo for l in lists) and any(l[0] >= hi for l in lists)
        assert any(l[0] < lo <= l[-1] for l in lists) and any(l[0] < hi <= l[-1] for l in lists)


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("first_id", rw.FIRST_IDS)
def test_rows_host_equals_python(hand_made, whole, first_id, threads):
    lists, src = hand_made[first_id]
    keep = [x.copy() for x in src]
    for lo, hi in rw.WINDOWS:
        a, b = first_id + lo, first_id + hi
        want = whole[first_id] if (lo, hi) == (0, rw.N) else rw.expected_rows(lists, src[1], a, b)
        got = indexio.rows_host(*src, rw.N, first_id=first_id, lo=a, hi=b, threads=threads)
        assert _eq(got, want), (lo, hi)
        assert len(got[1]) == hi - lo + 1 and int(got[1][0]) == 0
        assert _eq(got, _cut(whole[first_id], lo, hi)), (lo, hi)          # slice consistency: the whole index, cut
    assert all(np.array_equal(x, y) for x, y in zip(src, keep))          # the source arrays are untouched
    assert _eq(indexio.rows_host(*src, rw.N, first_id=first_id, threads=threads), whole[first_id])      # the default window


def test_rows_host_empty_index():
    h, off = indexio.rows_host(np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(1, np.uint64), 10, first_id=3)
    assert len(h) == 0 and h.dtype == np.uint32 and off.tolist() == [0] * 11 and off.dtype == np.uint64


def test_rows_host_equals_the_lists_the_oracle_indexes():
    """the oracle's index over a dozen small structures, transposed, is the per-structure sorted-unique lists it was built from"""
    from folddisco_amd import synth
    structs = packed_to_oracle_structs(synth.to_packed(synth.generate(12, seed=31)))
    h, off = oracle.hash_batch(structs)
    ix = oracle.build_index(structs)[0]
    src = (ix.values().copy(), ix.hashes().copy(), ix.offsets().copy())
    want = (np.asarray(h, np.uint32), np.asarray(off, np.uint64))
    assert len(want[0]) > 1000 and _eq(indexio.rows_host(*src, 12, threads=2), want)
    assert _eq(indexio.rows_host(*src, 12, lo=3, hi=9), _cut(want, 3, 9))
    ix2 = oracle.build_index_from_lists(h, off)
    assert np.array_equal(ix2.values(), src[0]) and np.array_equal(ix2.offsets(), src[2])      # build_index_from_lists' input is what came back


def test_rows_host_errors():
    v, h, o = rw.pack([[100, 105], [101, 300], [120]])
    good = indexio.rows_host(v, h, o, 1000, first_id=100)
    for lo, hi in ((99, 200), (100, 1101), (200, 150)):                     # a window past the index, or backwards
        with pytest.raises(ValueError, match=r"\(-1\)"):
            indexio.rows_host(v, h, o, 1000, first_id=100, lo=lo, hi=hi)
    for lists in ([[100, 105], [101, 1100], [120]], [[100, 105], [99, 300], [120]]):      # one id outside [first_id, first_id + n), in a walked list
        with pytest.raises(ValueError, match=r"\(-1\)"):
            indexio.rows_host(*rw.pack(lists), 1000, first_id=100, lo=100, hi=400)
    bad = o.copy()
    bad[1], bad[2] = o[2], o[1]                                             # offsets that do not ascend
    with pytest.raises(ValueError, match=r"\(-1\)"):
        indexio.rows_host(v, h, bad, 1000, first_id=100)
    bad = o.copy()
    bad[-1] += 1                                                            # the last list leaves the value bytes
    with pytest.raises(ValueError, match=r"\(-1\)"):
        indexio.rows_host(v, h, bad, 1000, first_id=100)
    with pytest.raises(ValueError, match=r"\(-1\)"):                        # a varint without an end inside its list
        indexio.rows_host(np.array([0x05, 0x80, 0x80], np.uint8), np.array([1], np.uint32), np.array([0, 3], np.uint64), 1000)
    assert _eq(indexio.rows_host(v, h, o, 1000, first_id=100), good)        # the good call still passes
    assert good[0].tolist() == [1, 4, 1, 7, 4] and np.nonzero(np.diff(good[1].astype(np.int64)))[0].tolist() == [0, 1, 5, 20, 200]


# ---- the command
N = 40


@pytest.fixture(scope="module")
def lists():
    """sorted unique hashes of every structure of a small synthetic batch as CSR: the oracle's, no product code"""
    from folddisco_amd import synth
    return oracle.hash_batch(packed_to_oracle_structs(synth.to_packed(synth.generate(N, seed=31))))


def _write_index(prefix, lists, **type_kw):
    h, off = lists
    ix = oracle.build_index_from_lists(h, off)
    indexio.write_index_files(prefix, ix.values().copy(), ix.hashes().copy(), ix.offsets().copy())
    indexio.save_lookup_py(prefix + ".lookup", [f"s{k}" for k in range(N)], 50 + np.arange(N, dtype=np.uint64), np.full(N, 80.5, np.float32))
    indexio.save_type(prefix + ".type", N, **type_kw)


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


def test_rows_host_command(tmp_path, lists, no_device, capsys):
    pre, out = str(tmp_path / "ix"), str(tmp_path / "OUT.npz")
    _write_index(pre, lists)
    h, off = np.asarray(lists[0], np.uint32), np.asarray(lists[1], np.uint64)
    assert _status(["rows", "--host", "-i", pre, "-o", out, "-t", "3", "--window", "7", "--verify", "-v"]) == 0
    cap = capsys.readouterr()
    longest = int(np.diff(off.astype(np.int64)).max())
    assert cap.out == f"[OK] {out}: {N} structures, {len(h)} hashes, longest row {longest}\n" and "6 window(s)" in cap.err
    z = np.load(out)
    assert sorted(z.files) == ["hashes", "ids", "row_off", "tids"]
    assert _eq((z["hashes"], z["row_off"]), (h, off)) and z["ids"].tolist() == list(range(N)) and z["tids"].tolist() == [f"s{k}" for k in range(N)]
    assert _status(["rows", "--host", "-i", pre, "-o", out, "--range", "13:31", "--window", "5"]) == 0      # over an existing output
    z = np.load(out)
    assert _eq((z["hashes"], z["row_off"]), _cut((h, off), 13, 31)) and z["ids"].tolist() == list(range(13, 31))
    assert _status(["rows", "--host", "-i", pre, "-o", out, "--range", "9:9"]) == 0
    z = np.load(out)
    assert len(z["hashes"]) == 0 and z["row_off"].tolist() == [0] and len(z["tids"]) == 0
    order = [31, 2, 39, 17, 2, 0]                                           # the file's order is kept, a repeat included
    (tmp_path / "t.txt").write_text("".join(f"s{k}\n" for k in order) + "\n")
    assert _status(["rows", "--host", "-i", pre, "-o", out, "--tids", str(tmp_path / "t.txt"), "--window", "16"]) == 0
    z = np.load(out)
    assert z["ids"].tolist() == order and z["tids"].tolist() == [f"s{k}" for k in order]
    assert np.array_equal(z["hashes"], np.concatenate([h[int(off[k]):int(off[k + 1])] for k in order]))
    assert np.array_equal(np.diff(z["row_off"].astype(np.int64)), np.array([int(off[k + 1] - off[k]) for k in order]))
    assert not [f for f in os.listdir(tmp_path) if "rows-tmp" in f]


def test_rows_refusals_before_any_device_call(tmp_path, lists, no_device, capsys):
    pre, out = str(tmp_path / "ix"), str(tmp_path / "OUT.npz")
    _write_index(pre, lists)
    (tmp_path / "t.txt").write_text("s3\nnope\ns5\n")
    names = sorted(os.listdir(tmp_path))
    assert _status(["rows", "-i", pre, "-o", out, "--tids", str(tmp_path / "t.txt")]) == 1           # an unknown tid
    assert "nope" in capsys.readouterr().out
    assert _status(["rows", "-i", pre, "-o", out, "--tids", str(tmp_path / "missing.txt")]) == 2     # missing files
    assert _status(["rows", "-i", str(tmp_path / "nope"), "-o", out]) == 2
    assert _status(["rows", "-i", pre, "-o", out, "--range", "5:41"]) == 1                            # a range past the index
    assert _status(["rows", "-i", pre, "-o", out, "--range", "5:9", "--tids", str(tmp_path / "t.txt")]) == 1
    assert _status(["rows", "-i", pre]) == 1                                                          # no -o
    bad = str(tmp_path / "bad")
    _write_index(bad, lists)
    with open(bad, "ab") as f:
        f.write(b"\x01")                                                                              # what check_index_files finds
    names = sorted(os.listdir(tmp_path))
    capsys.readouterr()
    assert _status(["rows", "-i", bad, "-o", out]) == 1 and "inconsistent" in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path)) == names


def test_verify_structures_refusals_before_any_device_call(tmp_path, lists, no_device, capsys):
    pre = str(tmp_path / "ix")
    _write_index(pre, lists)
    assert _status(["verify", "-i", pre, "--structures"]) == 1                                        # no store and no --coords
    assert _status(["verify", "-i", pre, "--structures", "--coords", str(tmp_path / "nope.coords")]) == 1
    assert _status(["verify", "-i", pre, "--structures", "--host"]) == 1                              # no host hasher
    mb = str(tmp_path / "mb")
    _write_index(mb, lists, multiple_bins=[(16, 4), (8, 3)])
    assert _status(["verify", "-i", mb, "--structures"]) == 1                                         # --multiple-bins
    capsys.readouterr()
    # without the flag: what it printed before, the report alone
    assert _status(["verify", "-i", pre, "--host"]) == 0
    v, h, o = indexio.read_index_files(pre)
    assert capsys.readouterr().out == f"{indexio.verify_host(v, h, o, N)}\n"
