"""Index update (fdgpu_index_remove, FolddiscoIndex.remove / append, `python -m folddisco_amd update`): an updated index is byte for byte the
index a fresh build over the resulting structure list gives — kept structures in their old order, then the added ones."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import oracle
from tests.helpers import SER, packed_to_oracle_structs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def synth180():
    from folddisco_amd import synth
    return synth.to_packed(synth.generate(180, seed=31))


def _items(ps, idx=None):
    off = ps.res_off.astype(np.int64)
    return [dict(n_xyz=ps.n_xyz[off[s]:off[s + 1]], ca_xyz=ps.ca_xyz[off[s]:off[s + 1]], cb_xyz=ps.cb_xyz[off[s]:off[s + 1]], aa=ps.aa[off[s]:off[s + 1]])
            for s in (range(ps.n_struct) if idx is None else idx)]


def _subset(ps, idx):
    import folddisco_amd as fd
    return fd.PackedStructures.concat(_items(ps, idx))


def _same(a, b):
    av, ah, ao = a.export()
    bv, bh, bo = b.export()
    assert a.num_hashes == b.num_hashes and a.value_len == b.value_len and a.num_postings == b.num_postings
    assert np.array_equal(ah, bh) and np.array_equal(ao, bo) and np.array_equal(av, bv)


def _masks(n):
    rng = np.random.Generator(np.random.PCG64(11))
    m = {"all": np.ones(n, bool)}
    m["drop_first"] = np.r_[False, np.ones(n - 1, bool)]
    m["drop_last"] = np.r_[np.ones(n - 1, bool), False]
    m["every_other"] = np.arange(n) % 2 == 0
    m["random30"] = rng.random(n) >= 0.3
    one = np.zeros(n, bool)
    one[n // 3] = True
    m["only_one"] = one
    return m


@pytest.mark.parametrize("first_id", [0, 7, 16380, 2100000])
@pytest.mark.parametrize("mask", ["all", "drop_first", "drop_last", "every_other", "random30", "only_one"])
def test_remove_equals_fresh_build(ctx, synth180, mask, first_id):
    """keep masks x first ids whose absolute / delta varints cross the 1/2/3/4-byte boundaries"""
    import folddisco_amd as fd
    keep = _masks(synth180.n_struct)[mask]
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180), first_id=first_id)
    pr = ix.remove(keep)
    want = fd.FolddiscoIndex.build(ctx, ctx.upload(_subset(synth180, np.nonzero(keep)[0])), first_id=first_id)
    assert pr.n_structures == int(keep.sum()) and pr.first_id == first_id
    _same(pr, want)
    _same(ix, fd.FolddiscoIndex.build(ctx, ctx.upload(synth180), first_id=first_id))      # the source index is untouched


def test_remove_drops_hashes_only_removed_structures_held(ctx, synth180):
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180))
    _, h, _ = ix.export()
    lists = ix.get_entries(h)
    single = sorted({int(l[0]) for l in lists if len(l) == 1})
    assert len(single) >= 3
    keep = np.ones(synth180.n_struct, bool)
    keep[single[:3]] = False
    pr = ix.remove(keep)
    gone = sum(1 for l in lists if set(l.tolist()) <= set(single[:3]))
    assert gone > 0 and pr.num_hashes == ix.num_hashes - gone
    _same(pr, fd.FolddiscoIndex.build(ctx, ctx.upload(_subset(synth180, np.nonzero(keep)[0]))))


def test_remove_equals_oracle(ctx, synth180):
    """independent of the GPU build: the pruned bytes equal the oracle's index over the kept structures' hash lists"""
    import folddisco_amd as fd
    keep = _masks(synth180.n_struct)["random30"]
    pr = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180)).remove(keep)
    h, off = oracle.hash_batch(packed_to_oracle_structs(_subset(synth180, np.nonzero(keep)[0])))
    oix = oracle.build_index_from_lists(h, off)
    v, hh, o = pr.export()
    assert np.array_equal(hh, oix.hashes()) and np.array_equal(o, oix.offsets()) and np.array_equal(v, oix.values())


def test_remove_long_lists_and_wide_hashes(ctx):
    """lists of ~1,500 ids (many 256-byte decode steps) and the 2^32 hash space (a structure with an overflowed hash)"""
    import folddisco_amd as fd
    from folddisco_amd import synth
    one = synth.to_packed(synth.generate(1, seed=77, lengths=np.array([60])))
    n = 1500
    item = dict(n_xyz=one.n_xyz, ca_xyz=one.ca_xyz, cb_xyz=one.cb_xyz, aa=one.aa)
    far = dict(n_xyz=one.n_xyz.copy(), ca_xyz=one.ca_xyz.copy(), cb_xyz=one.cb_xyz.copy(), aa=one.aa)
    far["cb_xyz"][7] = np.float32(3.0e38)
    items = [item] * 700 + [far] + [item] * (n - 701)
    ps = fd.PackedStructures.concat(items)
    rng = np.random.Generator(np.random.PCG64(3))
    keep = rng.random(n) >= 0.1
    keep[900:1000] = False                               # one whole contiguous run
    keep[700] = True                                     # the overflowed hash stays
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(ps), first_id=100)
    pr = ix.remove(keep)
    want = fd.FolddiscoIndex.build(ctx, ctx.upload(fd.PackedStructures.concat([items[s] for s in np.nonzero(keep)[0]])), first_id=100)
    v, h, o = want.export()
    assert h.max() >= (1 << 30) and np.diff(o).max() > 1200
    _same(pr, want)


def test_remove_from_loaded_index(ctx, synth180):
    """an index that came through fdgpu_index_load carries no per-list last ids"""
    import folddisco_amd as fd
    keep = _masks(synth180.n_struct)["random30"]
    v, h, o = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180)).export()
    loaded = fd.FolddiscoIndex.load(ctx, h, o, v, synth180.n_struct)
    pr = loaded.remove(keep)
    _same(pr, fd.FolddiscoIndex.build(ctx, ctx.upload(_subset(synth180, np.nonzero(keep)[0]))))
    lv, lh, lo = loaded.export()                         # still valid
    assert np.array_equal(lv, v) and np.array_equal(lh, h) and np.array_equal(lo, o)


def test_remove_then_append_equals_one_build(ctx, synth180):
    import folddisco_amd as fd
    from folddisco_amd import synth
    add = synth.to_packed(synth.generate(37, seed=99))
    keep = _masks(synth180.n_struct)["random30"]
    for first_id in (0, 300):
        ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180), first_id=first_id)
        up = ix.remove(keep).append(ctx, ctx.upload(add))
        kept = _subset(synth180, np.nonzero(keep)[0])
        allps = fd.PackedStructures.concat(_items(synth180, np.nonzero(keep)[0]) + _items(add))
        want = fd.FolddiscoIndex.build(ctx, ctx.upload(allps), first_id=first_id)
        assert up.n_structures == kept.n_struct + add.n_struct and up.first_id == first_id
        _same(up, want)
    v, h, o = want.export()
    rng = np.random.Generator(np.random.PCG64(5))
    qh = rng.choice(h, 40, replace=False).astype(np.uint32)
    qi = rng.integers(0, 4, len(qh)).astype(np.uint32)
    qj = rng.integers(0, 4, len(qh)).astype(np.uint32)
    pen = fd.length_penalty(np.diff(allps.res_off).astype(np.uint64), 0.5)
    assert fd.count_query(ctx, up, qh, qi, qj, pen, as_array=True).tobytes() == fd.count_query(ctx, want, qh, qi, qj, pen, as_array=True).tobytes()


def test_update_20500_structures(ctx):
    """1 % removed and 1 % appended at 20,500 structures, compared outright with a fresh build"""
    import folddisco_amd as fd
    from folddisco_amd import synth
    n, k = 20500, 205
    ps = synth.to_packed(synth.generate(n, seed=2024))
    add = synth.to_packed(synth.generate(k, seed=2025))
    rng = np.random.Generator(np.random.PCG64(17))
    keep = np.ones(n, bool)
    keep[rng.choice(n, k, replace=False)] = False
    up = fd.FolddiscoIndex.build(ctx, ctx.upload(ps)).remove(keep).append(ctx, ctx.upload(add))
    allps = fd.PackedStructures.concat(_items(ps, np.nonzero(keep)[0]) + _items(add))
    _same(up, fd.FolddiscoIndex.build(ctx, ctx.upload(allps)))


def test_remove_abi_errors(ctx, synth180):
    import ctypes as C
    import folddisco_amd as fd
    from folddisco_amd._lib import u8p
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180))
    h = C.c_void_p()
    none = np.zeros(synth180.n_struct, np.uint8)
    assert ctx.L.fdgpu_index_remove(ctx.h, ix.h, none.ctypes.data_as(u8p), len(none), C.byref(h)) == -1      # FDGPU_EINVAL: nothing kept
    short = np.ones(synth180.n_struct - 1, np.uint8)
    assert ctx.L.fdgpu_index_remove(ctx.h, ix.h, short.ctypes.data_as(u8p), len(short), C.byref(h)) == -1    # n_keep mismatch
    assert not h.value
    with pytest.raises(fd.FdgpuError):
        ix.remove(np.zeros(synth180.n_struct, bool))


# ---- CLI
def _cli(args, cwd, check=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "folddisco_amd", *args], cwd=cwd, env=env, capture_output=True, text=True)
    if check:
        assert r.returncode == 0, r.stderr
    return r


def _files(prefix):
    return [open(prefix + ext, "rb").read() for ext in ("", ".offset", ".lookup", ".type")]


@pytest.mark.parametrize("build_flags", [[], ["-y", "FolddiscoAngle", "--multiple-bins", "8-32,4-12"]])
def test_cli_update_equals_index(tmp_path, build_flags):
    """index four serine peptidases, update --remove one and -p the fifth == index over the kept files and the added one"""
    by = {os.path.basename(p)[:-4]: p for p in SER}
    names = sorted(by)                                   # 1azw 1ju3 1l7a 1pq5 4cha: sorted walk order = kept + added
    first, added, gone = names[:4], names[4], names[1]
    for d, ns in (("in_first", first), ("in_add", [added]), ("in_fresh", [n for n in names if n != gone])):
        (tmp_path / d).mkdir()
        for nm in ns:
            shutil.copy(by[nm], tmp_path / d / (nm + ".pdb"))
    (tmp_path / "gone.txt").write_text(gone + "\n")
    _cli(["index", "-p", "in_first", "-i", "up", "--id", "basename_without_ext", *build_flags], tmp_path)
    _cli(["index", "-p", "in_fresh", "-i", "fresh", "--id", "basename_without_ext", *build_flags], tmp_path)
    _cli(["update", "-i", "up", "--remove", "gone.txt", "-p", "in_add", "--id", "basename_without_ext"], tmp_path)
    assert _files(str(tmp_path / "up")) == _files(str(tmp_path / "fresh"))
    assert not [f for f in os.listdir(tmp_path) if "update-tmp" in f]
    q = os.path.join(GOLDEN, "query", "serine_peptidase.txt")
    outs = [_cli(["query", "-q", q, "-i", str(tmp_path / p), "--skip-match", "--header"], GOLDEN).stdout for p in ("up", "fresh")]
    assert outs[0] == outs[1] and len(outs[0].splitlines()) > 1


def test_cli_update_refusals(tmp_path):
    """unknown tids: exit 1, files unchanged; -p on a Foldcomp-built index is refused; --remove on one keeps the kept rows' db_keys"""
    (tmp_path / "db").mkdir()
    for p in SER[:3]:
        shutil.copy(p, tmp_path / "db" / os.path.basename(p))
    _cli(["index", "-p", "db", "-i", "ix", "--id", "basename_without_ext"], tmp_path)
    pre = str(tmp_path / "ix")
    before = _files(pre)
    mt = [os.stat(pre + ext).st_mtime_ns for ext in ("", ".offset", ".lookup", ".type")]
    (tmp_path / "bad.txt").write_text("nosuch1\n" + os.path.basename(SER[0])[:-4] + "\nnosuch2\n")
    r = _cli(["update", "-i", "ix", "--remove", "bad.txt"], tmp_path, check=False)
    assert r.returncode == 1 and "nosuch1" in r.stderr and "nosuch2" in r.stderr
    assert _files(pre) == before and [os.stat(pre + ext).st_mtime_ns for ext in ("", ".offset", ".lookup", ".type")] == mt
    # Foldcomp-built index
    fc = os.path.join(GOLDEN, "foldcomp", "example_db")
    _cli(["index", "-p", fc, "-i", "fcix"], tmp_path)
    r = _cli(["update", "-i", "fcix", "-p", "db"], tmp_path, check=False)
    assert r.returncode != 0 and "Foldcomp" in r.stderr
    rows = [l.rstrip("\n").split("\t") for l in open(tmp_path / "fcix.lookup")]
    assert len(rows) >= 3
    (tmp_path / "fcgone.txt").write_text(rows[1][1] + "\n")
    _cli(["update", "-i", "fcix", "--remove", "fcgone.txt", "-o", "fcix2"], tmp_path)
    new = [l.rstrip("\n").split("\t") for l in open(tmp_path / "fcix2.lookup")]
    kept = [r for r in rows if r[1] != rows[1][1]]
    assert [r[0] for r in new] == [str(i) for i in range(len(kept))]
    assert [r[1:] for r in new] == [r[1:] for r in kept]               # tid, nres, plddt and the database key verbatim
    assert _files(str(tmp_path / "fcix"))[2] == "".join("\t".join(r) + "\n" for r in rows).encode()   # -o: the input is untouched
