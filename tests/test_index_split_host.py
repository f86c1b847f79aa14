"""Index resharding on the host, no GPU: fdgpu_split_host (indexio.split_host) against the oracle, its round trip through merge_subindices, and the
validation of `python -m folddisco_amd reshard`, which runs before any device call (and the whole command with --host)."""
import os

import numpy as np
import pytest

import oracle
from folddisco_amd import indexio
from tests.helpers import packed_to_oracle_structs

N = 180
UNEVEN = [0, 1, 2, 50, 50, 51, 179, 180]      # single structures in parts of their own, an empty part, one wide part


@pytest.fixture(scope="module")
def lists():
    """sorted unique hashes of every structure of synth180 as CSR: the oracle's, no product code"""
    from folddisco_amd import synth
    return oracle.hash_batch(packed_to_oracle_structs(synth.to_packed(synth.generate(N, seed=31))))


def _oracle_index(lists, first_id=0, lo=None, hi=None):
    """the oracle's index over the lists with structure s at id first_id + s; with [lo, hi): every structure outside it emptied, the ids stay absolute"""
    h, off = lists
    n = np.diff(off.astype(np.int64))
    keep = np.ones(len(n), bool)
    if lo is not None:
        ids = first_id + np.arange(len(n))
        keep = (ids >= lo) & (ids < hi)
    h2 = h[np.repeat(keep, n)]
    off2 = np.concatenate([np.zeros(first_id + 1, np.int64), np.cumsum(np.where(keep, n, 0))]).astype(np.uint64)
    ix = oracle.build_index_from_lists(h2, off2)
    return ix.values().copy(), ix.hashes().copy(), ix.offsets().copy()


def _bounds(w, first_id=0):
    return indexio.shard_bounds(w, N) + np.uint64(first_id)


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


CASES = [(w, 0) for w in (1, 2, 3, 7, 200)] + [("uneven", 0), (3, 16380), (7, 2100000), ("uneven", 16380)]


@pytest.mark.parametrize("w,first_id", CASES)
def test_split_host_equals_oracle_parts(lists, w, first_id):
    b = np.array(UNEVEN, np.uint64) + np.uint64(first_id) if w == "uneven" else _bounds(w, first_id)
    whole = _oracle_index(lists, first_id)
    if len(b) - 1 > 64:                                   # W = 200: more parts than one call takes, so the cut is made in two rounds
        outer = np.r_[b[:-1:64], b[-1]]
        parts = []
        for k, chunk in enumerate(indexio.split_host(*whole, bounds=outer, first_id=first_id, threads=2)):
            parts += indexio.split_host(*chunk, bounds=b[64 * k: 64 * k + 65], first_id=int(outer[k]), threads=2)
    else:
        parts = indexio.split_host(*whole, bounds=b, first_id=first_id, threads=3)
    assert len(parts) == len(b) - 1
    for r, p in enumerate(parts):
        lo, hi = int(b[r]), int(b[r + 1])
        want = _oracle_index(lists, first_id, lo, hi)
        assert _eq(p, want), f"part {r} [{lo}, {hi})"
        rep = indexio.verify_host(*p, n_structures=hi - lo, first_id=lo)
        assert rep.ok, f"part {r}: {rep}"
        if hi == lo:
            assert len(p[0]) == 0 and len(p[1]) == 0 and p[2].tolist() == [0]
    if len(parts) <= 64:
        assert _eq(indexio.merge_subindices(parts), whole)


def test_split_host_shard_bounds_are_shard_range():
    from folddisco_amd.indexio import shard_range
    for w, n in ((1, 5), (3, 180), (7, 180), (64, 10), (8, 20500)):
        b = indexio.shard_bounds(w, n)
        assert [(int(b[r]), int(b[r + 1])) for r in range(w)] == [shard_range(r, w, n) for r in range(w)]


def _long_list_index():
    """the input of test_remove_long_lists_and_wide_hashes as oracle lists: 1,500 copies of one structure, one of them with an overflowed hash"""
    from folddisco_amd import synth
    one = synth.to_packed(synth.generate(1, seed=77, lengths=np.array([60])))
    far_cb = one.cb_xyz.copy()
    far_cb[7] = np.float32(3.0e38)
    a = oracle.structure_from_packed(one.n_xyz, one.ca_xyz, one.cb_xyz, one.aa)
    b = oracle.structure_from_packed(one.n_xyz, one.ca_xyz, far_cb, one.aa)
    ha, hb = oracle.hash_batch([a])[0], oracle.hash_batch([b])[0]
    n = 1500
    per = [hb if s == 700 else ha for s in range(n)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.uint64)
    return (np.concatenate(per), off), n


def _numpy_index(lists, first_id=0, lo=None, hi=None):
    """_oracle_index in numpy, for hashes of 2^30 and above (the oracle's table, like the reference's, ends there): postings sorted by (hash, id),
    LEB128 of the absolute first id and of the deltas behind it"""
    h, off = lists
    n = np.diff(off.astype(np.int64))
    ids = np.repeat(first_id + np.arange(len(n), dtype=np.int64), n)
    hh = h.astype(np.int64)
    if lo is not None:
        m = (ids >= lo) & (ids < hi)
        ids, hh = ids[m], hh[m]
    order = np.lexsort((ids, hh))
    ids, hh = ids[order], hh[order]
    first = np.r_[True, hh[1:] != hh[:-1]] if len(hh) else np.zeros(0, bool)
    val = np.where(first, ids, ids - np.r_[0, ids[:-1]]) if len(hh) else ids
    nb = np.ones(len(val), np.int64)
    for k in range(1, 5):
        nb += val >= (1 << (7 * k))
    start = np.concatenate([[0], np.cumsum(nb)])
    out = np.zeros(int(start[-1]), np.uint8)
    for k in range(5):
        m = nb > k
        out[start[:-1][m] + k] = ((val[m] >> (7 * k)) & 0x7f) | np.where(nb[m] > k + 1, 0x80, 0)
    return out, hh[first].astype(np.uint32), np.r_[start[:-1][first], start[-1]].astype(np.uint64)


def test_numpy_index_is_the_oracles(lists):
    assert _eq(_numpy_index(lists, 16380), _oracle_index(lists, 16380)) and _eq(_numpy_index(lists, 7, 50, 120), _oracle_index(lists, 7, 50, 120))


def test_split_host_long_lists_round_trip():
    lists, n = _long_list_index()
    whole = _numpy_index(lists, 100)
    assert whole[1].max() >= (1 << 30) and np.diff(whole[2].astype(np.int64)).max() > 1200
    assert indexio.verify_host(*whole, n_structures=n, first_id=100).ok
    for b in (indexio.shard_bounds(8, n) + np.uint64(100), np.array([100, 101, 102, 800, 801, 1599, 1600], np.uint64)):
        parts = indexio.split_host(*whole, bounds=b, first_id=100, threads=4)
        assert _eq(indexio.merge_subindices(parts), whole)
        for r, p in enumerate(parts):
            assert _eq(p, _numpy_index(lists, 100, int(b[r]), int(b[r + 1])))
            assert indexio.verify_host(*p, n_structures=int(b[r + 1] - b[r]), first_id=int(b[r])).ok


def test_split_host_bad_arguments(lists):
    whole = _oracle_index(lists)
    for bad in ([0, 100, 50, 180], [1, 90, 180], [0], list(range(0, 65)) + [180], [0, 90, 170]):
        with pytest.raises(ValueError):
            indexio.split_host(*whole, bounds=np.array(bad, np.uint64))
    with pytest.raises(ValueError):                       # first id of the bounds is not the index's
        indexio.split_host(*whole, bounds=np.array([0, 180], np.uint64), first_id=5)
    assert len(indexio.split_host(*whole, bounds=np.array([0] * 64 + [180], np.uint64))) == 64      # 64 parts are taken, 63 of them empty


# ---- the command
def _write_index(prefix, arrays, n):
    indexio.write_index_files(prefix, *arrays)
    indexio.save_lookup_py(prefix + ".lookup", [f"s{k}" for k in range(n)], np.full(n, 50, np.uint64), np.full(n, 80.5, np.float32))
    indexio.save_type(prefix + ".type", n)


@pytest.fixture
def no_device(monkeypatch):
    import folddisco_amd as fd

    def boom(*a, **k):
        raise AssertionError("a device was touched by a host-side reshard or before its validation ended")
    monkeypatch.setattr(fd, "Context", boom)


def _status(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


def test_reshard_refusals_before_any_device_call(tmp_path, lists, no_device):
    pre = str(tmp_path / "ix")
    _write_index(pre, _oracle_index(lists), N)
    names = sorted(os.listdir(tmp_path))
    assert _status(["reshard", "-i", pre, "--to", "1"]) == 1                       # --from == --to
    assert _status(["reshard", "-i", pre, "--to", "0"]) == 1
    assert _status(["reshard", "-i", pre, "--to", "65"]) == 1
    assert _status(["reshard", "-i", pre, "--from", "65", "--to", "2"]) == 1
    assert _status(["reshard", "-i", str(tmp_path / "nope"), "--to", "2"]) == 2    # missing files
    assert _status(["reshard", "-i", pre, "--from", "2", "--to", "1"]) == 2        # no shard files of 2
    bad = str(tmp_path / "bad")
    _write_index(bad, _oracle_index(lists), N)
    with open(bad + ".lookup", "a") as f:
        f.write("7\textra\t1\t1\t7\n")                                             # a row whose id is not its row number
    assert _status(["reshard", "-i", bad, "--to", "2"]) == 1
    _write_index(bad, _oracle_index(lists), N)
    with open(bad, "ab") as f:
        f.write(b"\x01")                                                           # last offset != size of the value file
    assert _status(["reshard", "-i", bad, "--to", "2"]) == 1
    _write_index(bad, _oracle_index(lists), N)
    with open(bad + ".offset", "ab") as f:
        f.write(b"\x00" * 8)                                                       # header disagrees with the file's size
    assert _status(["reshard", "-i", bad, "--to", "2"]) == 1
    assert sorted(f for f in os.listdir(tmp_path) if not f.startswith("bad")) == names


def test_reshard_host_round_trip(tmp_path, lists, no_device, capsys):
    pre, out = str(tmp_path / "ix"), str(tmp_path / "OUT")
    whole = _oracle_index(lists)
    _write_index(pre, whole, N)
    assert _status(["reshard", "--host", "-i", pre, "--to", "3", "--verify", "-t", "2"]) == 0
    assert "[OK]" in capsys.readouterr().out
    b = indexio.shard_bounds(3, N)
    for r in range(3):
        got = indexio.read_index_files(f"{pre}.shard{r}of3")
        assert _eq(got, _oracle_index(lists, 0, int(b[r]), int(b[r + 1])))
    assert _status(["reshard", "--host", "-i", pre, "--from", "3", "--to", "1", "-o", out]) == 0
    for ext in ("", ".offset", ".lookup", ".type"):
        assert open(out + ext, "rb").read() == open(pre + ext, "rb").read(), ext
    assert _status(["reshard", "--host", "-i", pre, "--from", "3", "--to", "2", "-o", out]) == 0      # shards -> shards of another count
    b = indexio.shard_bounds(2, N)
    for r in range(2):
        assert _eq(indexio.read_index_files(f"{out}.shard{r}of2"), _oracle_index(lists, 0, int(b[r]), int(b[r + 1])))
    assert not [f for f in os.listdir(tmp_path) if "reshard-tmp" in f]
