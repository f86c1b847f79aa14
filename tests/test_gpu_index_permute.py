"""Index reorder on the device (fdgpu_index_permute, FolddiscoIndex.permute, `python -m folddisco_amd reorder`): a permuted index is byte for byte
the build over the same structures taken in the new order, on every list class of csrc/k_permute.hip (LDS sort, LDS bitmap, global-memory slab)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from folddisco_amd import indexio
from tests import permute_cases as pc
from tests.helpers import SER

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 180
PERMS = pc.permutations()


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


def _build(ctx, items, seq, first_id):
    """a fresh build over the batch's structures taken in the order seq with the given first id"""
    import folddisco_amd as fd
    return fd.FolddiscoIndex.build(ctx, ctx.upload(fd.PackedStructures.concat([items[s] for s in seq])), first_id=first_id)


def ctx_structs(ix):
    return int(ix.ctx.L.fdgpu_index_num_structures(ix.h))


def _same(a, b):
    av, ah, ao = a.export()
    bv, bh, bo = b.export()
    assert a.num_hashes == b.num_hashes and a.value_len == b.value_len and a.num_postings == b.num_postings
    assert a.first_id == b.first_id and a.n_structures == b.n_structures
    assert ctx_structs(a) == ctx_structs(b)
    assert np.array_equal(ah, bh) and np.array_equal(ao, bo) and np.array_equal(av, bv)


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


def _perm180(kind):
    k = np.arange(N)
    return {"reversal": N - 1 - k, "random": np.random.Generator(np.random.PCG64(77)).permutation(N), "rotate1": (k + 1) % N, "identity": k}[kind].astype(np.uint32)


def _seq(p):
    """the order of the structures after new_id = p: position j holds the structure k with p[k] = j"""
    return [int(s) for s in pc.inverse(p)]


# ---- 1. permute == a fresh build in the new order
@pytest.mark.parametrize("first_id", [0, 16300, 2097100])
@pytest.mark.parametrize("kind", ["reversal", "random", "rotate1", "identity"])
def test_permute_equals_fresh_build(ctx, items, kind, first_id):
    p = _perm180(kind)
    src = _build(ctx, items, range(N), first_id)
    before = src.export()
    got = src.permute(p)
    _same(got, _build(ctx, items, _seq(p), first_id))
    assert _eq(src.export(), before) and src.first_id == first_id          # the source index is unchanged


# ---- 2. hand-made lists, independent of the GPU build: device == host == Python, on every list class
SETTINGS = {      # name -> (environment, the stages that must have run)
    "default": ({}, {"permute_write_sort", "permute_write_lds"}),
    "sort_bytes_lowered": ({"FDGPU_PERM_SORT_BYTES": str(pc.SORT_BYTES_LOW)}, {"permute_write_sort", "permute_write_lds"}),
    "lds_bits_lowered": ({"FDGPU_PERM_LDS_BITS": str(pc.LDS_BITS_LOW)}, {"permute_write_sort", "permute_write_slab"}),
    "both_lowered": ({"FDGPU_PERM_SORT_BYTES": str(pc.SORT_BYTES_LOW), "FDGPU_PERM_LDS_BITS": str(pc.LDS_BITS_LOW)}, {"permute_write_sort", "permute_write_slab"}),
}


def _timed_permute(ctx, ix, p):
    ctx.enable_timing(True)
    try:
        got = ix.permute(p)
        stages = {n: b for n, _, b in ctx.last_timings()}
    finally:
        ctx.enable_timing(False)
    return got, stages


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("name", sorted(PERMS))
@pytest.mark.parametrize("first_id", pc.FIRST_IDS)
def test_permute_hand_made_lists(ctx, monkeypatch, first_id, name, setting):
    import folddisco_amd as fd
    env, must_run = SETTINGS[setting]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    p = PERMS[name]
    lists, (v, h, o), want = pc.case(first_id, name)
    assert int(o[-1]) == len(v)                                            # the last list ends on the last value byte
    ix = fd.FolddiscoIndex.load(ctx, h, o, v, pc.N, first_id=first_id)      # loaded: no per-list last ids
    got, stages = _timed_permute(ctx, ix, p)
    assert must_run <= set(stages) and not {"permute_write_lds", "permute_write_slab"} <= set(stages), stages
    lens = np.diff(o.astype(np.int64))
    bound = pc.SORT_BYTES_LOW if "FDGPU_PERM_SORT_BYTES" in env else pc.SORT_BYTES
    bitmap = "permute_sizes_slab" if "FDGPU_PERM_LDS_BITS" in env else "permute_sizes_lds"
    assert stages[bitmap] >= int(lens[lens > bound].sum()) > 0 and (lens <= bound).any()      # the lists past the boundary went to the bitmap class
    assert _eq(got.export(), want)
    if setting == "default":
        assert _eq(indexio.permute_host(v, h, o, p, first_id=first_id, threads=2), want)
    assert got.first_id == first_id and got.num_postings == ix.num_postings == sum(len(l) for l in lists) and ctx_structs(got) == pc.N
    assert _eq(ix.export(), (v, h, o))
    back = got.permute(pc.inverse(p))                                      # a permuted index (pooled, with last ids) as the source
    assert _eq(back.export(), (v, h, o))
    rep = got.verify()
    assert rep.ok and rep.n_postings == ix.num_postings and rep.n_lists == len(lists) and rep.max_id == first_id + pc.N - 1, str(rep)


def test_permute_through_export_and_load(ctx, items):
    import folddisco_amd as fd
    p = _perm180("random")
    src = _build(ctx, items, range(N), 16300)                              # built: carries last ids
    v, h, o = src.export()
    loaded = fd.FolddiscoIndex.load(ctx, h, o, v, N, first_id=16300)        # loaded: carries none
    _same(loaded.permute(p), src.permute(p))


def test_permute_empty_index(ctx):
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.load(ctx, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint8), 10, first_id=500)
    got = ix.permute(np.arange(10)[::-1].copy())
    v, h, o = got.export()
    assert len(v) == 0 and len(h) == 0 and o.tolist() == [0] and got.first_id == 500 and ctx_structs(got) == 10


# ---- 3. round trip and downstream calls
@pytest.mark.parametrize("first_id", [0, 16300])
def test_permuted_index_round_trip_verify_split_entries(ctx, items, first_id):
    p = _perm180("random")
    src = _build(ctx, items, range(N), first_id)
    got = src.permute(p)
    assert _eq(got.permute(pc.inverse(p)).export(), src.export())
    r0, rep = src.verify(), got.verify()
    assert rep.ok and r0.ok and rep.max_id == r0.max_id and rep.n_postings == r0.n_postings and rep.n_lists == r0.n_lists, str(rep)
    seq = _seq(p)
    b = indexio.shard_bounds(3, N)
    for r, part in enumerate(got.split(b + np.uint64(first_id))):
        _same(part, _build(ctx, items, seq[int(b[r]):int(b[r + 1])], first_id + int(b[r])))
    v, h, o = src.export()
    lens = np.diff(o.astype(np.int64))
    pick = np.unique(np.concatenate([h[:3], h[-3:], h[np.argsort(lens)[-3:]], h[len(h) // 2: len(h) // 2 + 3]]))
    for a, g in zip(src.get_entries(pick), got.get_entries(pick)):
        assert g.tolist() == sorted(first_id + int(p[int(x) - first_id]) for x in a) and len(a) > 0


# ---- 4. errors leave nothing behind and the context usable
def test_permute_errors(ctx, items):
    import folddisco_amd as fd
    from folddisco_amd._lib import u32p
    src = _build(ctx, items, range(N), 0)
    ident = np.arange(N, dtype=np.uint32)

    def call(ix, arr, n):
        out = C.c_void_p(1)
        rc = ctx.L.fdgpu_index_permute(ctx.h, ix.h, arr.ctypes.data_as(u32p), n, C.byref(out))
        return rc, out.value
    assert call(src, ident, N - 1) == (-1, None)                           # n differs from the index's structures
    twice = ident.copy()
    twice[5] = 6
    assert call(src, twice, N) == (-1, None)                               # a repeated value
    big = ident.copy()
    big[5] = N
    assert call(src, big, N) == (-1, None)                                 # a value >= n
    with pytest.raises(ValueError):
        src.permute(ident[:-1])
    with pytest.raises(fd.FdgpuError):
        src.permute(twice)
    # an index loaded with fewer structures than its ids need: found while decoding, in the sort class and in the bitmap class
    for lists, n in (([[0, 5], [3, 12], [9]], 10), ([list(range(3000)), [7]], 1000)):
        v, h, o = pc.pack(lists)
        low = fd.FolddiscoIndex.load(ctx, h, o, v, n)
        assert call(low, np.arange(n, dtype=np.uint32), n) == (-1, None)
        with pytest.raises(ValueError, match=r"\(-1\)"):
            indexio.permute_host(v, h, o, np.arange(n, dtype=np.uint32))
    p = _perm180("reversal")
    _same(src.permute(p), _build(ctx, items, _seq(p), 0))                  # a good permute still passes
    good = fd.FolddiscoIndex.load(ctx, *[pc.pack([[0, 5], [3, 12], [9]])[k] for k in (1, 2, 0)], 13)
    assert _eq(good.permute(np.arange(13)[::-1].copy()).export(), pc.pack([[7, 12], [0, 9], [3]]))


# ---- 5. the command
def _cli(args, cwd, check=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "folddisco_amd", *args], cwd=cwd, env=env, capture_output=True, text=True)
    if check:
        assert r.returncode == 0, r.stderr
    return r


def _files(prefix):
    return {ext: open(str(prefix) + ext, "rb").read() for ext in ("", ".offset", ".lookup", ".type")}


def test_cli_reorder_end_to_end(tmp_path):
    """index five files in one directory (A) and the same files under B/v .. B/z so that the sorted recursive walk of B is the reverse of A's
    (--id pdb: the tids do not depend on the directory): reorder -i ixA into B's order writes ixB's four files"""
    (tmp_path / "A").mkdir()
    names = sorted(os.path.basename(p) for p in SER)
    assert len(names) == 5
    for p in SER:
        shutil.copy(p, tmp_path / "A" / os.path.basename(p))
        sub = tmp_path / "B" / "zyxwv"[names.index(os.path.basename(p))]
        sub.mkdir(parents=True)
        shutil.copy(p, sub / os.path.basename(p))
    _cli(["index", "-p", "A", "-i", "ixA", "--id", "pdb"], tmp_path)
    _cli(["index", "-p", "B", "-i", "ixB", "--id", "pdb", "-r"], tmp_path)
    col = lambda prefix: [r.split("\t")[1] for r in open(tmp_path / (prefix + ".lookup"))]
    assert col("ixB") == col("ixA")[::-1]
    (tmp_path / "orderB.txt").write_text("".join(t + "\n" for t in col("ixB")))
    (tmp_path / "orderA.txt").write_text("".join(t + "\n" for t in col("ixA")))
    want, start = _files(tmp_path / "ixB"), _files(tmp_path / "ixA")
    r = _cli(["reorder", "-i", "ixA", "--order", "orderB.txt", "-o", "OUT", "-v"], tmp_path)
    assert r.stdout.startswith("[OK] OUT: 5 structures reordered (4 moved), lists / postings / bytes: ") and len(r.stdout.strip().splitlines()) == 1
    assert "device" in r.stderr and f"-> {len(want[''])}" in r.stderr
    _cli(["reorder", "-i", "ixA", "--order", "orderB.txt", "-o", "OUTV", "--verify"], tmp_path)
    assert _files(tmp_path / "OUT") == want and _files(tmp_path / "OUTV") == want and _files(tmp_path / "ixA") == start
    for ext in start:
        shutil.copy(tmp_path / ("ixA" + ext), tmp_path / ("ixC" + ext))
    _cli(["reorder", "-i", "ixC", "--by", "tid", "--desc"], tmp_path)                          # in place
    assert _files(tmp_path / "ixC") == want
    _cli(["reorder", "-i", "ixC", "--order", "orderA.txt"], tmp_path)                          # and back
    assert _files(tmp_path / "ixC") == start
    (tmp_path / "short.txt").write_text("".join(t + "\n" for t in col("ixA")[1:]))
    r = _cli(["reorder", "-i", "ixA", "--order", "short.txt", "-o", "OUT2"], tmp_path, check=False)
    assert r.returncode == 1 and "missing" in r.stdout
    assert not [f for f in os.listdir(tmp_path) if f.startswith("OUT2") or "reorder-tmp" in f]
