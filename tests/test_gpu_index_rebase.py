"""Index join on the device (fdgpu_index_rebase, FolddiscoIndex.rebase, `python -m folddisco_amd merge`): a rebased index is byte for byte the build
over the same structures at the new first id, and rebase + merge joins indices that were built separately, each with ids from 0."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from folddisco_amd import indexio
from tests import rebase_cases as rc
from tests.helpers import SER

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


@pytest.fixture(scope="module")
def items(synth180):
    ps = synth180
    off = ps.res_off.astype(np.int64)
    return [dict(n_xyz=ps.n_xyz[off[s]:off[s + 1]], ca_xyz=ps.ca_xyz[off[s]:off[s + 1]], cb_xyz=ps.cb_xyz[off[s]:off[s + 1]], aa=ps.aa[off[s]:off[s + 1]])
            for s in range(ps.n_struct)]


def _build(ctx, items, lo, hi, first_id):
    """a fresh build over structures lo .. hi - 1 of the batch with the given first id"""
    import folddisco_amd as fd
    return fd.FolddiscoIndex.build(ctx, ctx.upload(fd.PackedStructures.concat(items[lo:hi])), first_id=first_id)


def _same(a, b):
    av, ah, ao = a.export()
    bv, bh, bo = b.export()
    assert a.num_hashes == b.num_hashes and a.value_len == b.value_len and a.num_postings == b.num_postings
    assert a.first_id == b.first_id and a.n_structures == b.n_structures
    assert ctx_structs(a) == ctx_structs(b)
    assert np.array_equal(ah, bh) and np.array_equal(ao, bo) and np.array_equal(av, bv)


def ctx_structs(ix):
    return int(ix.ctx.L.fdgpu_index_num_structures(ix.h))


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


# ---- 1. rebase == a fresh build; with 180 structures every pair has a varint boundary (127/128, 16383/16384, 2^21) inside one of the two id ranges
@pytest.mark.parametrize("a,b", [(0, 0), (0, 100), (100, 0), (0, 16300), (16300, 7), (7, 2097100), (2097100, 16380), (16380, 2100000)])
def test_rebase_equals_fresh_build(ctx, items, a, b):
    src = _build(ctx, items, 0, N, a)
    before = src.export()
    got = src.rebase(b)
    _same(got, _build(ctx, items, 0, N, b))
    assert _eq(src.export(), before) and src.first_id == a                 # the source index is unchanged
    _same(src, _build(ctx, items, 0, N, a))


# ---- 2. hand-made lists, independent of the GPU build: device == host == Python
@pytest.fixture(scope="module")
def hand_made():
    return {f: rc.make_lists(f) for f in sorted({f for f, _ in rc.CASES})}


@pytest.mark.parametrize("first_id,shift", rc.CASES)
def test_rebase_hand_made_lists(ctx, hand_made, first_id, shift):
    import folddisco_amd as fd
    lists = hand_made[first_id]
    v, h, o = rc.pack(lists)
    assert int(o[-1]) == len(v)                                            # the last list ends on the last value byte
    ix = fd.FolddiscoIndex.load(ctx, h, o, v, rc.N_STRUCTURES, first_id=first_id)
    got = ix.rebase(first_id + shift)
    want = rc.shifted(lists, shift)
    assert _eq(got.export(), want)
    assert _eq(indexio.rebase_host(v, h, o, first_id, first_id + shift, rc.N_STRUCTURES, threads=2), want)
    assert got.first_id == first_id + shift and got.num_postings == ix.num_postings == sum(len(l) for l in lists)
    assert _eq(ix.export(), (v, h, o))
    back = got.rebase(first_id)                                            # a rebased index (pooled, made by the copy kernel) as the source
    assert _eq(back.export(), (v, h, o))


def test_rebase_empty_index(ctx):
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.load(ctx, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint8), 10)
    got = ix.rebase(500)
    v, h, o = got.export()
    assert len(v) == 0 and len(h) == 0 and o.tolist() == [0] and got.first_id == 500 and ctx_structs(got) == 10


# ---- 3. the join
def _join(ctx, items, bounds, through_load):
    import folddisco_amd as fd
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        p = _build(ctx, items, int(lo), int(hi), 0)                        # every part built on its own, ids from 0
        if through_load:                                                   # ... and through export / load: no per-list last ids
            v, h, o = p.export()
            p = fd.FolddiscoIndex.load(ctx, h, o, v, int(hi - lo))
        parts.append(p.rebase(int(lo)))
    return fd.FolddiscoIndexSet(parts).merge()


@pytest.mark.parametrize("w,through_load", [(2, False), (64, False), (2, True), (7, True)])
def test_join_equals_single_build(ctx, items, w, through_load):
    _same(_join(ctx, items, indexio.shard_bounds(w, N), through_load), _build(ctx, items, 0, N, 0))


# ---- 4. downstream calls accept the result
def test_rebased_index_verifies_and_splits(ctx, items):
    src = _build(ctx, items, 0, N, 0)
    r0 = src.verify()
    got = src.rebase(16300)
    rep = got.verify()
    assert rep.ok and r0.ok and rep.max_id == r0.max_id + 16300 and rep.n_postings == r0.n_postings and rep.n_lists == r0.n_lists, str(rep)
    b = indexio.shard_bounds(3, N) + np.uint64(16300)
    for r, p in enumerate(got.split(b)):
        lo, hi = int(b[r]) - 16300, int(b[r + 1]) - 16300
        _same(p, _build(ctx, items, lo, hi, int(b[r])))
    b = indexio.shard_bounds(5, N)
    for r, p in enumerate(src.split(b)):                                   # a split part made stand-alone
        _same(p.rebase(0), _build(ctx, items, int(b[r]), int(b[r + 1]), 0))


# ---- 5. errors leave nothing behind and the context usable
def test_rebase_errors(ctx, items):
    import folddisco_amd as fd
    src = _build(ctx, items, 0, N, 0)
    out = C.c_void_p(1)
    assert ctx.L.fdgpu_index_rebase(ctx.h, src.h, (1 << 32) - 179, C.byref(out)) == -4 and not out.value      # FDGPU_ERANGE
    with pytest.raises(fd.FdgpuError):
        src.rebase((1 << 32) - 179)
    # a list that starts below the declared first_id, moved downwards: a damaged index
    v, h, o = rc.pack([[100, 105], [7, 300], [120]])
    low = fd.FolddiscoIndex.load(ctx, h, o, v, 1000, first_id=100)
    out = C.c_void_p(1)
    assert ctx.L.fdgpu_index_rebase(ctx.h, low.h, 0, C.byref(out)) == -1 and not out.value                    # FDGPU_EINVAL
    with pytest.raises(ValueError, match=r"\(-1\)"):
        indexio.rebase_host(v, h, o, 100, 0, 1000)
    _same(src.rebase(100), _build(ctx, items, 0, N, 100))                  # a good rebase still passes
    good = fd.FolddiscoIndex.load(ctx, *[rc.pack([[100, 105], [107, 300], [120]])[k] for k in (1, 2, 0)], 1000, first_id=100)
    assert _eq(good.rebase(0).export(), rc.pack([[0, 5], [7, 200], [20]]))


# ---- 6. the command
def _cli(args, cwd, check=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "folddisco_amd", *args], cwd=cwd, env=env, capture_output=True, text=True)
    if check:
        assert r.returncode == 0, r.stderr
    return r


def test_cli_merge_end_to_end(tmp_path):
    """index two directories on their own and all their files together (--id pdb: the tids do not depend on the directory; the sorted order of
    ALL is A's files, then B's): merge -i A B writes ALL's four files"""
    split = {"A": ("1azw", "1ju3", "1l7a"), "B": ("1pq5", "4cha")}
    for d in ("A", "B", "ALL"):
        (tmp_path / d).mkdir()
    for p in SER:
        stem = os.path.basename(p)[:-4]
        (d,) = [k for k, names in split.items() if stem in names]
        shutil.copy(p, tmp_path / d / os.path.basename(p))
        shutil.copy(p, tmp_path / "ALL" / os.path.basename(p))
    for d in ("A", "B", "ALL"):
        _cli(["index", "-p", d, "-i", "ix" + d, "--id", "pdb"], tmp_path)
    r = _cli(["merge", "-i", "ixA", "ixB", "-o", "OUT", "-v"], tmp_path)
    assert r.stdout.startswith("[OK] OUT: 2 inputs, 5 structures, lists / postings / bytes: ") and len(r.stdout.strip().splitlines()) == 1
    assert "0 duplicate tid(s)" in r.stderr and "device" in r.stderr
    _cli(["merge", "-i", "ixA", "ixB", "-o", "OUTV", "--verify"], tmp_path)
    for out in ("OUT", "OUTV"):
        for ext in ("", ".offset", ".lookup", ".type"):
            assert open(tmp_path / (out + ext), "rb").read() == open(tmp_path / ("ixALL" + ext), "rb").read(), (out, ext)
    _cli(["index", "-p", "B", "-i", "ixB8", "--id", "pdb", "-d", "8"], tmp_path)
    r = _cli(["merge", "-i", "ixA", "ixB8", "-o", "OUT2"], tmp_path, check=False)
    assert r.returncode == 1 and "num_bin_dist" in r.stdout
    assert not [f for f in os.listdir(tmp_path) if f.startswith("OUT2") or "merge-tmp" in f]
