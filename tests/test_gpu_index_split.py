"""Index resharding on the device (fdgpu_index_split, FolddiscoIndex.split, `python -m folddisco_amd reshard`): part r of a split is byte for byte
the index a build over the structures of its id range gives with first_id = the range's start, and the merge of the parts is the source."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import oracle
from folddisco_amd import indexio
from tests.helpers import SER, packed_to_oracle_structs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 180


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def synth180():
    from folddisco_amd import synth
    return synth.to_packed(synth.generate(N, seed=31))


def _items(ps, idx=None):
    off = ps.res_off.astype(np.int64)
    return [dict(n_xyz=ps.n_xyz[off[s]:off[s + 1]], ca_xyz=ps.ca_xyz[off[s]:off[s + 1]], cb_xyz=ps.cb_xyz[off[s]:off[s + 1]], aa=ps.aa[off[s]:off[s + 1]])
            for s in (range(ps.n_struct) if idx is None else idx)]


def _build_range(ctx, items, lo, hi, first_id):
    """a fresh build over structures lo - first_id .. hi - first_id - 1 with first_id = lo (an empty range: a build over an empty batch)"""
    import folddisco_amd as fd
    return fd.FolddiscoIndex.build(ctx, ctx.upload(fd.PackedStructures.concat(items[lo - first_id: hi - first_id])), first_id=lo)


def _same(a, b):
    av, ah, ao = a.export()
    bv, bh, bo = b.export()
    assert a.num_hashes == b.num_hashes and a.value_len == b.value_len and a.num_postings == b.num_postings
    assert a.first_id == b.first_id and a.n_structures == b.n_structures
    assert np.array_equal(ah, bh) and np.array_equal(ao, bo) and np.array_equal(av, bv)


@pytest.mark.parametrize("first_id", [0, 7, 16380, 2100000])
@pytest.mark.parametrize("w", [2, 3, 7, 64])
def test_split_equals_fresh_builds(ctx, synth180, w, first_id):
    import folddisco_amd as fd
    items = _items(synth180)
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180), first_id=first_id)
    b = indexio.shard_bounds(w, N) + np.uint64(first_id)
    parts = ix.split(b)
    assert len(parts) == w
    for r, p in enumerate(parts):
        _same(p, _build_range(ctx, items, int(b[r]), int(b[r + 1]), first_id))
    _same(ix, fd.FolddiscoIndex.build(ctx, ctx.upload(synth180), first_id=first_id))      # the source index is untouched


def test_split_one_part_is_a_copy_and_empty_parts(ctx, synth180):
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180), first_id=5)
    (p,) = ix.split([5, 5 + N])
    _same(p, ix)
    b = np.array([5, 5, 6, 100, 100, 100, 185, 185], np.uint64)
    parts = ix.split(b)
    items = _items(synth180)
    for r, p in enumerate(parts):
        _same(p, _build_range(ctx, items, int(b[r]), int(b[r + 1]), 5))
    assert parts[0].num_hashes == 0 and parts[0].export()[2].tolist() == [0]
    _same(fd.FolddiscoIndexSet(parts).merge(), ix)


def test_split_device_equals_host_equals_oracle(ctx, synth180):
    """independent of the GPU build: the parts equal fdgpu_split_host's and the oracle's index over the lists with the other structures emptied"""
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180))
    b = indexio.shard_bounds(7, N)
    dev = [p.export() for p in ix.split(b)]
    host = indexio.split_host(*ix.export(), bounds=b, threads=2)
    h, off = oracle.hash_batch(packed_to_oracle_structs(synth180))
    n = np.diff(off.astype(np.int64))
    for r in range(7):
        keep = (np.arange(N) >= int(b[r])) & (np.arange(N) < int(b[r + 1]))
        oix = oracle.build_index_from_lists(h[np.repeat(keep, n)], np.concatenate([[0], np.cumsum(np.where(keep, n, 0))]).astype(np.uint64))
        for got in (dev[r], host[r]):
            assert np.array_equal(got[1], oix.hashes()) and np.array_equal(got[2], oix.offsets()) and np.array_equal(got[0], oix.values())


def test_split_merge_round_trip_loaded_and_pruned(ctx, synth180):
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180), first_id=300)
    b = indexio.shard_bounds(5, N) + np.uint64(300)
    parts = ix.split(b)
    _same(fd.FolddiscoIndexSet(parts).merge(), ix)
    # an index that came through fdgpu_index_load carries no per-list last ids
    v, h, o = ix.export()
    loaded = fd.FolddiscoIndex.load(ctx, h, o, v, N, first_id=300)
    for p, q in zip(loaded.split(b), parts):
        _same(p, q)
    lv, lh, lo = loaded.export()
    assert np.array_equal(lv, v) and np.array_equal(lh, h) and np.array_equal(lo, o)
    # a pruned index: remove, then split == builds over the kept subsets
    keep = np.random.Generator(np.random.PCG64(11)).random(N) >= 0.3
    kept = [it for it, k in zip(_items(synth180), keep) if k]
    pr = ix.remove(keep)
    b2 = indexio.shard_bounds(4, len(kept)) + np.uint64(300)
    for r, p in enumerate(pr.split(b2)):
        _same(p, _build_range(ctx, kept, int(b2[r]), int(b2[r + 1]), 300))


def test_split_long_lists_and_wide_hashes(ctx):
    """lists of ~1,500 ids that cross every bound (many 256-byte decode steps, several piece heads per step) and the 2^32 hash space"""
    import folddisco_amd as fd
    from folddisco_amd import synth
    one = synth.to_packed(synth.generate(1, seed=77, lengths=np.array([60])))
    n = 1500
    item = dict(n_xyz=one.n_xyz, ca_xyz=one.ca_xyz, cb_xyz=one.cb_xyz, aa=one.aa)
    far = dict(n_xyz=one.n_xyz.copy(), ca_xyz=one.ca_xyz.copy(), cb_xyz=one.cb_xyz.copy(), aa=one.aa)
    far["cb_xyz"][7] = np.float32(3.0e38)
    items = [item] * 700 + [far] + [item] * (n - 701)
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(fd.PackedStructures.concat(items)), first_id=100)
    v, h, o = ix.export()
    assert h.max() >= (1 << 30) and np.diff(o.astype(np.int64)).max() > 1200
    singles = np.array([100, 101, 102, 103, 800, 801, 802, 1599, 1600], np.uint64)      # structures 100, 101, 102, 800 (the wide one), 801, 1599 alone
    for b in (indexio.shard_bounds(8, n) + np.uint64(100), singles, indexio.shard_bounds(64, n) + np.uint64(100)):
        parts = ix.split(b)
        for r, p in enumerate(parts):
            _same(p, _build_range(ctx, items, int(b[r]), int(b[r + 1]), 100))
            assert p.verify().ok
        _same(fd.FolddiscoIndexSet(parts).merge(), ix)


def test_split_20500_structures(ctx):
    import folddisco_amd as fd
    from folddisco_amd import synth
    n = 20500
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth.to_packed(synth.generate(n, seed=2024))))
    parts = ix.split(indexio.shard_bounds(8, n))
    for p in parts:
        rep = p.verify()                                  # with the part's own first_id / n_structures: ID_RANGE proves no id landed in the wrong shard
        assert rep.ok and rep.n_postings == p.num_postings and rep.n_lists == p.num_hashes, str(rep)
    assert sum(p.num_postings for p in parts) == ix.num_postings
    mv, mh, mo = fd.FolddiscoIndexSet(parts).merge().export()
    v, h, o = ix.export()
    assert np.array_equal(mh, h) and np.array_equal(mo, o) and np.array_equal(mv, v)


def test_split_abi_errors(ctx, synth180):
    import ctypes as C
    import folddisco_amd as fd
    from folddisco_amd._lib import u64p
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180))
    out = (C.c_void_p * 65)()

    def rc(bounds):
        b = np.array(bounds, np.uint64)
        code = ctx.L.fdgpu_index_split(ctx.h, ix.h, len(b) - 1, b.ctypes.data_as(u64p), out)
        assert not any(out[k] for k in range(65))
        return code
    assert rc([0, 100, 50, 180]) == -1 and rc([1, 90, 180]) == -1 and rc([0, 90, 170]) == -1 and rc([0]) == -1      # FDGPU_EINVAL
    assert rc(list(range(65)) + [180]) == -1                                                                        # 65 parts
    with pytest.raises(fd.FdgpuError):
        ix.split([0, 90, 181])
    # an index whose ids pass n_structures: the kernel sets the error bit, nothing is returned
    v, h, o = ix.export()
    short = fd.FolddiscoIndex.load(ctx, h, o, v, N - 10)
    b = np.array([0, 80, N - 10], np.uint64)
    assert ctx.L.fdgpu_index_split(ctx.h, short.h, 2, b.ctypes.data_as(u64p), out) == -1 and not out[0] and not out[1]


# ---- CLI
def _cli(args, cwd, check=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "folddisco_amd", *args], cwd=cwd, env=env, capture_output=True, text=True)
    if check:
        assert r.returncode == 0, r.stderr
    return r


def _pair(prefix):
    return [open(prefix + ext, "rb").read() for ext in ("", ".offset")]


def test_cli_reshard_end_to_end(tmp_path, ctx):
    """index a small directory, reshard --to 2 == the files of builds over the two shard_range halves; 2 -> 3 == 1 -> 3; 3 -> 1 == the original.
    (The sharded `query` over the resharded files is not run here: the two-rank workers of tests/shard_query_worker.py build their own shards
    and cannot be pointed at existing files without editing them.)"""
    import folddisco_amd as fd
    from folddisco_amd import structure
    (tmp_path / "db").mkdir()
    for p in SER:
        shutil.copy(p, tmp_path / "db" / os.path.basename(p))
    _cli(["index", "-p", "db", "-i", "ix", "--id", "basename_without_ext"], tmp_path)
    pre = str(tmp_path / "ix")
    paths = sorted(str(tmp_path / "db" / f) for f in os.listdir(tmp_path / "db"))
    r = _cli(["reshard", "-i", "ix", "--to", "2", "--verify", "-v"], tmp_path)
    assert r.stdout.startswith("[OK]") and "left as they are" in r.stderr
    b = indexio.shard_bounds(2, len(paths))
    for k in range(2):
        ps = structure.read_packed(paths[int(b[k]): int(b[k + 1])])[0]
        fd.FolddiscoIndex.build(ctx, ctx.upload(ps), first_id=int(b[k])).save(str(tmp_path / f"want{k}"))
        assert _pair(f"{pre}.shard{k}of2") == _pair(str(tmp_path / f"want{k}"))
    _cli(["reshard", "-i", "ix", "--from", "2", "--to", "3", "-o", "via2"], tmp_path)
    _cli(["reshard", "-i", "ix", "--to", "3"], tmp_path)
    for k in range(3):
        assert _pair(f"{pre}.shard{k}of3") == _pair(str(tmp_path / f"via2.shard{k}of3"))
    _cli(["reshard", "-i", "ix", "--from", "3", "--to", "1", "-o", "OUT"], tmp_path)
    for ext in ("", ".offset", ".lookup", ".type"):
        assert open(str(tmp_path / "OUT") + ext, "rb").read() == open(pre + ext, "rb").read()
    assert os.path.exists(pre + ".shard0of2") and not [f for f in os.listdir(tmp_path) if "reshard-tmp" in f]
