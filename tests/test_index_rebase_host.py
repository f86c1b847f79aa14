"""Index join on the host, no GPU: fdgpu_rebase_host (indexio.rebase_host) against hand-made lists shifted in Python, the lookup / type helpers
of the join, and `python -m folddisco_amd merge`: its refusals, which come before any device call, and the whole command with --host."""
import os

import numpy as np
import pytest

import oracle
from folddisco_amd import indexio
from tests import rebase_cases as rc
from tests.helpers import packed_to_oracle_structs


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


@pytest.fixture(scope="module")
def hand_made():
    return {f: rc.make_lists(f) for f in sorted({f for f, _ in rc.CASES})}


def test_hand_made_index_has_the_edges(hand_made):
    """the shape the cases rely on: every head value, every byte length, and a last list that ends on the last value byte"""
    lists = hand_made[0]
    v, h, o = rc.pack(lists)
    assert {l[0] for l in lists} == set(rc.BASE_HEADS) and set(np.diff(o.astype(np.int64)).tolist()) == set(rc.LENGTHS)
    assert int(o[-1]) == len(v) and int(o[-1] - o[-2]) == 1 and max(rc.LENGTHS) > 4096
    assert indexio.verify_host(v, h, o, rc.N_STRUCTURES).ok
    assert [rc.decode(rc.encode(l)) for l in lists] == lists


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("first_id,shift", rc.CASES)
def test_rebase_host_equals_python(hand_made, first_id, shift, threads):
    lists = hand_made[first_id]
    src = rc.pack(lists)
    keep = [x.copy() for x in src]
    got = indexio.rebase_host(*src, first_id, first_id + shift, rc.N_STRUCTURES, threads=threads)
    assert _eq(got, rc.shifted(lists, shift))
    assert _eq(src, keep)                                                  # the source arrays are untouched
    assert indexio.verify_host(*got, n_structures=rc.N_STRUCTURES, first_id=first_id + shift).ok
    if shift:                                                              # and back again
        assert _eq(indexio.rebase_host(*got, first_id + shift, first_id, rc.N_STRUCTURES, threads=threads), src)


def test_rebase_host_empty_index():
    v, h, o = indexio.rebase_host(np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(1, np.uint64), 0, 100, 10)
    assert len(v) == 0 and len(h) == 0 and o.tolist() == [0]


def test_rebase_host_errors(hand_made):
    src = rc.pack(hand_made[0])
    with pytest.raises(ValueError, match=r"\(-4\)"):                       # FDGPU_ERANGE: the last id would need 33 bits
        indexio.rebase_host(*src, 0, (1 << 32) - rc.N_STRUCTURES + 1, rc.N_STRUCTURES)
    with pytest.raises(ValueError, match=r"\(-4\)"):
        indexio.rebase_host(*src, 0, (1 << 32) - 179, 180)
    # a list that starts below the declared first_id, moved downwards: a damaged index, FDGPU_EINVAL
    low = rc.pack([[100, 105], [7, 300], [120]])
    with pytest.raises(ValueError, match=r"\(-1\)"):
        indexio.rebase_host(*low, 100, 0, 1000)
    with pytest.raises(ValueError, match=r"\(-1\)"):                       # ... and a first id past the range, moved upwards
        indexio.rebase_host(*rc.pack([[100, 105], [2000]]), 100, 200, 1000)
    v, h, o = rc.pack([[100, 105], [101], [120]])
    bad = o.copy()
    bad[1], bad[2] = o[2], o[1]                                            # offsets that do not ascend
    with pytest.raises(ValueError, match=r"\(-1\)"):
        indexio.rebase_host(v, h, bad, 100, 0, 1000)
    bad = o.copy()
    bad[-1] += 1                                                           # the last list leaves the value bytes
    with pytest.raises(ValueError, match=r"\(-1\)"):
        indexio.rebase_host(v, h, bad, 100, 0, 1000)
    with pytest.raises(ValueError, match=r"\(-1\)"):                       # a first varint without an end inside its list
        indexio.rebase_host(np.array([0x80, 0x80, 0x80], np.uint8), np.array([1], np.uint32), np.array([0, 3], np.uint64), 0, 5, 1000)
    assert _eq(indexio.rebase_host(v, h, o, 100, 0, 1000), rc.pack([[0, 5], [1], [20]]))      # the good call still passes


def test_join_lookup_rows_file_built():
    a = indexio.lookup_rows(0, ["x", "y", "z"], [10, 20, 30], [80.5, 0.0, 91.25])
    b = indexio.lookup_rows(0, ["p", "x"], [40, 10], [70.0, 80.5])
    out = [r.rstrip("\n").split("\t") for r in indexio.join_lookup_rows([a, b], keep_db_keys=False)]
    assert [r[0] for r in out] == [r[4] for r in out] == ["0", "1", "2", "3", "4"]          # db_key follows the id
    assert [r[1:4] for r in out] == [r.rstrip("\n").split("\t")[1:4] for r in a + b]         # tid, nres and plddt verbatim, duplicates kept
    assert "".join(indexio.join_lookup_rows([a, b], False)) == "".join(indexio.lookup_rows(0, ["x", "y", "z", "p", "x"], [10, 20, 30, 40, 10],
                                                                                          [80.5, 0.0, 91.25, 70.0, 80.5]))


def test_join_lookup_rows_foldcomp_built():
    a = indexio.lookup_rows(0, ["x", "y"], [10, 20], [80.5, 0.0], db_keys=[17, 4])
    b = indexio.lookup_rows(0, ["p", "q", "r"], [40, 10, 5], [70.0, 80.5, 1.0], db_keys=[900, 3, 17])
    out = [r.rstrip("\n").split("\t") for r in indexio.join_lookup_rows([a, b], keep_db_keys=True)]
    assert [r[0] for r in out] == ["0", "1", "2", "3", "4"] and [r[4] for r in out] == ["17", "4", "900", "3", "17"]      # db_key kept
    assert [r[1:4] for r in out] == [r.rstrip("\n").split("\t")[1:4] for r in a + b]


def _type_text(tmp_path, n, **kw):
    p = str(tmp_path / "t.type")
    indexio.save_type(p, n, **kw)
    with open(p) as f:
        return f.read()


def test_check_joinable_names_the_key(tmp_path):
    base = _type_text(tmp_path, 10)
    assert indexio.check_joinable([base, _type_text(tmp_path, 99), _type_text(tmp_path, 3)]) is None      # chunk_size may differ
    assert indexio.check_joinable([base, _type_text(tmp_path, 10, nbin_dist=8)]) == "num_bin_dist"
    assert indexio.check_joinable([base, base, _type_text(tmp_path, 10, nbin_angle=3)]) == "num_bin_angle"
    assert indexio.check_joinable([base, _type_text(tmp_path, 10, grid_width=15.0)]) == "grid_width"
    assert indexio.check_joinable([base, _type_text(tmp_path, 10, hash_type="PDBMotif")]) == "hash_type"
    fc = _type_text(tmp_path, 10, input_format="FCZDB", foldcomp_db="a_foldcomp")
    assert indexio.check_joinable([base, fc]) in ("input_format", "foldcomp_db") and indexio.check_joinable([fc, base]) in ("input_format", "foldcomp_db")
    assert indexio.check_joinable([fc, _type_text(tmp_path, 5, input_format="FCZDB", foldcomp_db="b_foldcomp")]) == "foldcomp_db"
    assert indexio.check_joinable([base, _type_text(tmp_path, 10, multiple_bins=[(16, 4), (8, 3)])]) == "multiple_bin"


# ---- the command
N = 40


@pytest.fixture(scope="module")
def lists():
    """sorted unique hashes of every structure of a small synthetic batch as CSR: the oracle's, no product code"""
    from folddisco_amd import synth
    return oracle.hash_batch(packed_to_oracle_structs(synth.to_packed(synth.generate(N, seed=31))))


def _oracle_index(lists, lo, hi):
    """the oracle's index over structures lo .. hi - 1 of the batch, ids from 0"""
    h, off = lists
    off = off.astype(np.int64)
    ix = oracle.build_index_from_lists(h[off[lo]:off[hi]], (off[lo:hi + 1] - off[lo]).astype(np.uint64))
    return ix.values().copy(), ix.hashes().copy(), ix.offsets().copy()


def _write_index(prefix, arrays, lo, hi, **type_kw):
    indexio.write_index_files(prefix, *arrays)
    indexio.save_lookup_py(prefix + ".lookup", [f"s{k}" for k in range(lo, hi)], 50 + np.arange(lo, hi, dtype=np.uint64), np.full(hi - lo, 80.5, np.float32))
    indexio.save_type(prefix + ".type", hi - lo, **type_kw)


@pytest.fixture
def no_device(monkeypatch):
    import folddisco_amd as fd

    def boom(*a, **k):
        raise AssertionError("a device was touched by a host-side merge or before its validation ended")
    monkeypatch.setattr(fd, "Context", boom)


def _status(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


@pytest.mark.parametrize("cuts", [[0, 20, 40], [0, 1, 17, 40], [0, 13, 13 + 14, 40]])
def test_merge_host_end_to_end(tmp_path, lists, no_device, capsys, cuts):
    pres = []
    for k in range(len(cuts) - 1):
        pres.append(str(tmp_path / f"in{k}"))
        _write_index(pres[-1], _oracle_index(lists, cuts[k], cuts[k + 1]), cuts[k], cuts[k + 1])
    want, out = str(tmp_path / "want"), str(tmp_path / "OUT")
    _write_index(want, _oracle_index(lists, 0, N), 0, N)
    assert _status(["merge", "--host", "-i", *pres, "-o", out, "-t", "3", "--verify", "-v"]) == 0
    cap = capsys.readouterr()
    whole = indexio.read_index_files(want)
    assert cap.out.startswith(f"[OK] {out}: {len(pres)} inputs, {N} structures, lists / postings / bytes: {len(whole[1])} / ") and len(cap.out.strip().splitlines()) == 1
    assert "0 duplicate tid(s)" in cap.err
    for ext in ("", ".offset", ".lookup", ".type"):
        assert open(out + ext, "rb").read() == open(want + ext, "rb").read(), ext
    assert not [f for f in os.listdir(tmp_path) if "merge-tmp" in f]
    assert _status(["merge", "--host", "-i", *pres, "-o", out]) == 0      # over an existing output, without --verify
    assert open(out, "rb").read() == open(want, "rb").read()


def test_merge_refusals_before_any_device_call(tmp_path, lists, no_device, capsys):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _write_index(a, _oracle_index(lists, 0, 20), 0, 20)
    _write_index(b, _oracle_index(lists, 20, 40), 20, 40)
    names = sorted(os.listdir(tmp_path))
    out = str(tmp_path / "OUT")
    assert _status(["merge", "-i", a, "-o", out]) == 1                                   # one input
    assert _status(["merge", "-i", *([a, b] * 32 + [a]), "-o", out]) == 1                # 65 inputs
    assert _status(["merge", "-i", a, b]) == 1                                           # no -o
    assert _status(["merge", "-i", a, b, "-o", b]) == 1                                  # -o is an input
    assert _status(["merge", "-i", a, b, "-o", os.path.join(str(tmp_path), ".", "a")]) == 1
    assert _status(["merge", "-i", a, str(tmp_path / "nope"), "-o", out]) == 2           # a missing prefix
    assert sorted(os.listdir(tmp_path)) == names
    capsys.readouterr()
    fc = str(tmp_path / "fc")
    _write_index(fc, _oracle_index(lists, 20, 40), 20, 40, input_format="FCZDB", foldcomp_db="some_foldcomp")
    assert _status(["merge", "-i", a, fc, "-o", out]) == 1                               # file-built with Foldcomp-built
    assert "input_format" in capsys.readouterr().out
    fc2 = str(tmp_path / "fc2")
    _write_index(fc2, _oracle_index(lists, 0, 20), 0, 20, input_format="FCZDB", foldcomp_db="other_foldcomp")
    assert _status(["merge", "-i", fc, fc2, "-o", out]) == 1                             # two Foldcomp databases
    assert "foldcomp_db" in capsys.readouterr().out
    d8 = str(tmp_path / "d8")
    _write_index(d8, _oracle_index(lists, 20, 40), 20, 40, nbin_dist=8)
    assert _status(["merge", "-i", a, d8, "-o", out]) == 1                               # other hash settings: the key is named
    assert "num_bin_dist" in capsys.readouterr().out
    bad = str(tmp_path / "bad")
    _write_index(bad, _oracle_index(lists, 20, 40), 20, 40)
    with open(bad, "ab") as f:
        f.write(b"\x01")                                                                 # what check_index_files finds
    assert _status(["merge", "-i", a, bad, "-o", out]) == 1
    assert not [f for f in os.listdir(tmp_path) if f.startswith("OUT")]
