"""The coordinate store on the device and through the command line: the resident-batch operations (fdgpu_batch_select / _concat / _export,
Batch.select / .concat / .export) against numpy gathers byte for byte, their pairing with the id-mapping index operations (a rebuilt index and the
hashes pin the gathered coordinates), and `index --coords` / `coords` / `query` / `update` / `merge` / `reorder` / `reshard` over PREFIX.coords."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from folddisco_amd import indexio
from tests import coords_cases as cc
from tests.helpers import Q4CHA, SER

pytestmark = pytest.mark.gpu

QSTR = "B57,B102,C195"


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[True, False], ids=["cb_valid", "no_cb_valid"])
def copy_batch(ctx, request):
    """the hand-made batch, the 65,535-residue structure included, uploaded once with and once without cb_valid"""
    ps = cc.packed(with_long=True, with_cbv=request.param)
    return ps, ctx.upload(ps)


# ---- copies
def test_export_gives_the_uploaded_arrays_back(copy_batch):
    ps, b = copy_batch
    got = b.export()
    assert cc.same_bytes(got, cc.gather(ps, np.arange(ps.n_struct))) and (got.cb_valid is None) == (ps.cb_valid is None)


@pytest.mark.parametrize("name", list(cc.id_lists(16)))
def test_select_equals_the_numpy_gather(copy_batch, name):
    ps, b = copy_batch
    ids = cc.id_lists(ps.n_struct)[name]
    out = b.select(ids)
    assert out.n_struct == len(ids) == int(out.ctx.L.fdgpu_batch_num_structures(out.h))
    want = cc.gather(ps, ids)
    assert int(out.ctx.L.fdgpu_batch_num_residues(out.h)) == int(want["res_off"][-1])
    assert cc.same_bytes(out.export(), want), name
    assert cc.same_bytes(b.export(), cc.gather(ps, np.arange(ps.n_struct)))      # the source stays as it was


def test_select_of_a_select(copy_batch):
    ps, b = copy_batch
    first, second = cc.id_lists(ps.n_struct)["random"], np.array([3, 3, 0, 15, 7])
    assert cc.same_bytes(b.select(first).select(second).export(), cc.gather(ps, first[second]))


def test_concat_with_an_empty_part_and_mixed_cb_valid(ctx):
    import folddisco_amd as fd
    full, bare = cc.packed(False, True), cc.packed(False, False)
    bf, bb = ctx.upload(full), ctx.upload(bare)
    n = full.n_struct
    empty = bf.select([])
    a, c = bf.select(np.arange(0, 7)), bf.select(np.arange(7, n))
    assert cc.same_bytes(fd.Batch.concat([a, empty, c]).export(), cc.gather(full, np.arange(n)))
    assert cc.same_bytes(fd.Batch.concat([empty, empty]).export(), cc.gather(full, []))
    # without cb_valid everywhere: none in the result; in some parts only: those contribute ones
    assert fd.Batch.concat([bb, bb]).export().cb_valid is None
    got = fd.Batch.concat([bb.select(np.arange(0, 7)), c, bb.select([12])]).export()
    want = cc.gather(full, list(range(n)) + [12])
    cbv = want["cb_valid"].copy()
    off = full.res_off.astype(np.int64)
    cbv[:off[7]] = 1
    cbv[off[n]:] = 1
    want["cb_valid"] = cbv
    assert cc.same_bytes(got, want)
    with pytest.raises(fd.api.FdgpuError):
        fd.Batch.concat([bf])
    with pytest.raises(fd.api.FdgpuError):
        fd.Batch.concat([bf] * 65)


def test_select_error_paths_are_host_checks(ctx, copy_batch):
    """an id equal to n_struct is EINVAL, a gather of 2^32 residues ERANGE; *out stays NULL and nothing is launched or allocated"""
    ps, b = copy_batch
    L = ctx.L
    u32p = C.POINTER(C.c_uint32)
    out = C.c_void_p(0xdead)
    ids = np.array([0, ps.n_struct], np.uint32)
    assert L.fdgpu_batch_select(ctx.h, b.h, ids.ctypes.data_as(u32p), 2, C.byref(out)) == -1 and not out.value
    assert b"ids[1]" in L.fdgpu_last_error(ctx.h)
    # 65,538 times the 65,535-residue structure: 4,295,032,830 residues, past 2^32; 65,537 times: 2^32 - 1, which a batch refuses as well (the
    # limit of fdgpu_batch_upload).  Nothing of that size is allocated: the sum is taken on the host first
    long_id = ps.n_struct - 1
    for reps in (65538, 65537):
        out = C.c_void_p(0xdead)
        ids = np.full(reps, long_id, np.uint32)
        assert L.fdgpu_batch_select(ctx.h, b.h, ids.ctypes.data_as(u32p), reps, C.byref(out)) == -4 and not out.value
    assert b"2^32" in L.fdgpu_last_error(ctx.h)
    with pytest.raises(ValueError):
        b.select([-1])


# ---- pairing with the index operations
N_SYNTH = 600


@pytest.fixture(scope="module")
def paired(ctx):
    """about 600 synthetic structures followed by the edge lengths, uploaded once, and the index over them (default hash parameters)"""
    import folddisco_amd as fd
    from folddisco_amd import synth
    lens = np.concatenate([synth.sample_lengths(N_SYNTH, 5), np.array(cc.LENGTHS)]).astype(np.int64)
    ps = synth.to_packed(synth.generate(len(lens), seed=5, lengths=lens))
    b = ctx.upload(ps)
    return ps, b, fd.FolddiscoIndex.build(ctx, b)


def _same_index(a, b):
    av, ah, ao = a.export()
    bv, bh, bo = b.export()
    assert a.n_structures == b.n_structures and a.first_id == b.first_id and a.num_postings == b.num_postings
    assert np.array_equal(ah, bh) and np.array_equal(ao, bo) and np.array_equal(av, bv)
    assert len(ah) > 1000


def test_select_pairs_with_permute(ctx, paired):
    import folddisco_amd as fd
    ps, b, ix = paired
    new_id = np.random.Generator(np.random.PCG64(9)).permutation(ps.n_struct).astype(np.uint32)
    order = np.argsort(new_id)
    _same_index(fd.FolddiscoIndex.build(ctx, b.select(order)), ix.permute(new_id))


def test_select_pairs_with_remove(ctx, paired):
    import folddisco_amd as fd
    ps, b, ix = paired
    keep = np.random.Generator(np.random.PCG64(10)).random(ps.n_struct) < 0.7
    keep[-3:] = [True, False, True]
    _same_index(fd.FolddiscoIndex.build(ctx, b.select(np.nonzero(keep)[0])), ix.remove(keep))


def test_select_pairs_with_split(ctx, paired):
    import folddisco_amd as fd
    ps, b, ix = paired
    bounds = np.array([0, 200, 200, 601, ps.n_struct], np.uint64)
    for r, part in enumerate(ix.split(bounds)):
        built = fd.FolddiscoIndex.build(ctx, b.select(np.arange(int(bounds[r]), int(bounds[r + 1]))), first_id=int(bounds[r]))
        if bounds[r] == bounds[r + 1]:
            assert built.num_hashes == part.num_hashes == 0
        else:
            _same_index(built, part)


def test_concat_pairs_with_merge(ctx, paired):
    import folddisco_amd as fd
    ps, b, ix = paired
    n_a = 250
    a, c = b.select(np.arange(n_a)), b.select(np.arange(n_a, ps.n_struct))
    whole = fd.FolddiscoIndex.build(ctx, fd.Batch.concat([a, c]))
    _same_index(whole, fd.FolddiscoIndexSet([fd.FolddiscoIndex.build(ctx, a), fd.FolddiscoIndex.build(ctx, c, first_id=n_a)]).merge())
    _same_index(whole, ix)


def test_hashes_of_a_select_are_the_selected_rows(ctx, paired):
    import folddisco_amd as fd
    ps, b, ix = paired
    h, off = fd.get_geometric_hash_as_u32(ctx, b)
    ids = np.concatenate([np.random.Generator(np.random.PCG64(11)).permutation(ps.n_struct)[:150], np.arange(N_SYNTH, ps.n_struct), [N_SYNTH + 5, 3, 3]])
    hs, offs = fd.get_geometric_hash_as_u32(ctx, b.select(ids))
    assert np.array_equal(np.diff(offs.astype(np.int64)), (off[ids + 1] - off[ids]).astype(np.int64))
    assert np.array_equal(hs, np.concatenate([h[int(off[i]):int(off[i + 1])] for i in ids])) and len(hs) > 10000


# ---- command line, on the serine peptidases with the README's 4CHA query
def _cli(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


def _query(capsys, prefix, *extra):
    capsys.readouterr()
    rc = _cli(["query", "-p", Q4CHA, "-q", QSTR, "-i", prefix, *extra])
    return rc, capsys.readouterr().out


def _db(root, name, paths, numbered=False):
    d = os.path.join(str(root), name)
    os.makedirs(d)
    for k, p in enumerate(paths):
        shutil.copy(p, os.path.join(d, (f"{k:02d}_" if numbered else "") + os.path.basename(p)))
    return d


def _index(root, name, paths, coords=True, numbered=False):
    """`index [--coords]` over copies of the given files (numbered: named so that the walk takes them in the order given) -> prefix"""
    prefix = os.path.join(str(root), name)
    assert _cli(["index", "-p", _db(root, name + "_db", paths, numbered), "-i", prefix] + (["--coords"] if coords else [])) == 0
    return prefix


def _read(p):
    with open(p, "rb") as f:
        return f.read()


MODES = [[], ["--per-structure"], ["--per-structure", "--header"], ["--superpose"], ["--skip-ca-match"], ["--superpose", "--skip-ca-match", "--header"]]


@pytest.fixture(scope="module")
def ser_index(tmp_path_factory):
    root = tmp_path_factory.mktemp("coords_cli")
    return root, _index(root, "ix", SER)


def test_query_through_the_store_equals_the_parse_and_needs_no_structure_file(ser_index, capsys):
    root, prefix = ser_index
    assert sorted(os.listdir(root)) == ["ix", "ix.coords", "ix.lookup", "ix.offset", "ix.type", "ix_db"]
    want = {}
    for mode in MODES:
        rc0, parsed = _query(capsys, prefix, "--no-coords", *mode)
        rc1, stored = _query(capsys, prefix, *mode)
        assert rc0 == rc1 == 0 and stored == parsed and len(parsed.splitlines()) >= 5, mode
        want[tuple(mode)] = parsed
    # the modes are different tables (the from-hash mapping of --skip-ca-match may equal the processed one for this query)
    assert len({want[()], want[("--per-structure",)], want[("--per-structure", "--header")], want[("--superpose",)]}) == 4
    rc, explicit = _query(capsys, prefix, "--coords", prefix + ".coords")
    assert rc == 0 and explicit == want[()]
    # the structure files moved away: the store path is unchanged, the parse has nothing to read
    os.rename(os.path.join(root, "ix_db"), os.path.join(root, "ix_db_moved"))
    try:
        for mode in MODES:
            rc, stored = _query(capsys, prefix, *mode)
            assert rc == 0 and stored == want[tuple(mode)], mode
        rc, parsed = _query(capsys, prefix, "--no-coords")
        assert rc != 0 or parsed != want[()]
    finally:
        os.rename(os.path.join(root, "ix_db_moved"), os.path.join(root, "ix_db"))


def test_coords_on_a_plain_index_gives_the_store_of_index_coords(ser_index, tmp_path, capsys):
    root, prefix = ser_index
    plain = _index(tmp_path, "plain", SER, coords=False)
    assert sorted(os.listdir(tmp_path)) == ["plain", "plain.lookup", "plain.offset", "plain.type", "plain_db"]      # exactly the four files
    for ext in ("", ".offset"):
        assert _read(plain + ext) == _read(prefix + ext)
    assert _cli(["coords", "-i", plain, "-t", "2"]) == 0
    assert _read(plain + ".coords") == _read(prefix + ".coords")
    assert _cli(["verify", "-i", plain]) == 0 and f"[OK] {plain}.coords: 5 structures" in capsys.readouterr().out


def _store_follows(capsys, prefix, fresh):
    """the store at `prefix` equals the one a fresh `index --coords` wrote, its stamp holds, and the query through it equals the parse"""
    assert _read(prefix + ".coords") == _read(fresh + ".coords")
    indexio.CoordStore.open(prefix + ".coords", check_prefix=prefix)
    for mode in ([], ["--per-structure"]):
        rc0, parsed = _query(capsys, prefix, "--no-coords", *mode)
        rc1, stored = _query(capsys, prefix, *mode)
        assert rc0 == rc1 == 0 and stored == parsed and len(parsed.splitlines()) >= 4


def test_store_follows_reorder(tmp_path, capsys):
    prefix = _index(tmp_path, "ix", SER)
    nres = [int(l.split("\t")[2]) for l in open(prefix + ".lookup")]
    order = np.argsort(nres, kind="stable")
    assert order.tolist() != list(range(5))
    assert _cli(["reorder", "-i", prefix, "--by", "nres"]) == 0          # in place: the store is rewritten with the other files
    _store_follows(capsys, prefix, _index(tmp_path, "fresh", [SER[k] for k in order], numbered=True))


def test_store_follows_update(tmp_path, capsys):
    prefix = _index(tmp_path, "ix", SER)
    before = _read(prefix + ".coords")
    gone = [l.split("\t")[1] for l in open(prefix + ".lookup")][2]
    open(tmp_path / "rm.txt", "w").write(gone + "\n")
    assert _cli(["update", "-i", prefix, "--remove", str(tmp_path / "rm.txt")]) == 0
    _store_follows(capsys, prefix, _index(tmp_path, "fresh", SER[:2] + SER[3:], numbered=True))
    # appended structures: their arrays come from the parse the update does anyway
    assert _cli(["update", "-i", prefix, "-p", _db(tmp_path, "more", SER[2:3]), "-o", str(tmp_path / "grown")]) == 0
    _store_follows(capsys, str(tmp_path / "grown"), _index(tmp_path, "fresh2", SER[:2] + SER[3:] + SER[2:3], numbered=True))
    # the store from before the in-place update, kept aside and put back, is refused: no silent use, no silent fall-back to the files
    open(prefix + ".coords", "wb").write(before)
    rc, out = _query(capsys, prefix)
    assert rc == 1 and "coordinate store refused" in out and "lookup rows" in out
    rc, out = _query(capsys, prefix, "--no-coords")
    assert rc == 0 and len(out.splitlines()) >= 4


def test_store_follows_merge_and_reshard(tmp_path, capsys):
    a, b = _index(tmp_path, "a", SER[:3]), _index(tmp_path, "b", SER[3:])
    m = str(tmp_path / "m")
    assert _cli(["merge", "-i", a, b, "-o", m]) == 0
    whole = _index(tmp_path, "whole", SER)
    _store_follows(capsys, m, whole)
    # no input has a store: none is written
    os.remove(a + ".coords")
    os.remove(b + ".coords")
    assert _cli(["merge", "-i", a, b, "-o", str(tmp_path / "n")]) == 0 and not os.path.exists(str(tmp_path / "n.coords"))
    # reshard -o: the store goes with .lookup; written back as a single index it carries that index's stamp
    sh = str(tmp_path / "sh")
    assert _cli(["reshard", "-i", m, "--to", "2", "-o", sh]) == 0 and _read(sh + ".coords") == _read(m + ".coords")
    one = str(tmp_path / "one")
    assert _cli(["reshard", "-i", sh, "--from", "2", "--to", "1", "-o", one]) == 0
    _store_follows(capsys, one, whole)
