"""Index rows on the device (fdgpu_index_rows, FolddiscoIndex.rows, `python -m folddisco_amd rows`, `verify --structures`): the transposed
index of hand-made lists equals the host form and a pure-Python transposition at every radix-pass count, and the rows of a built, loaded,
merged, pruned, reordered or rebased index equal what the batch hasher gives for the same structures."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from folddisco_amd import indexio
from tests import rows_cases as rw
from tests.helpers import SER

pytestmark = pytest.mark.gpu

N = 180
WINDOWS = [(0, N), (0, 1), (N - 1, N), (57, 58), (60, 60), (13, 141)]


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


def _eq(a, b):
    return len(a) == len(b) == 2 and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def _cut(rows, lo, hi):
    h, off = rows
    return h[int(off[lo]):int(off[hi])], off[lo:hi + 1] - off[lo]


def _select(rows, ids):
    """the rows ids[k] of a CSR pair, in that order"""
    h, off = rows
    out = np.zeros(len(ids) + 1, np.uint64)
    out[1:] = np.cumsum([int(off[k + 1] - off[k]) for k in ids])
    return (np.concatenate([h[int(off[k]):int(off[k + 1])] for k in ids]) if len(ids) else np.zeros(0, np.uint32)), out


# ---- 1. hand-made lists, independent of the GPU build: device == host == Python, zero to four radix passes
@pytest.fixture(scope="module")
def hand_made():
    out = {}
    for f in rw.FIRST_IDS:
        lists = rw.lists(f)
        out[f] = (lists, rw.pack(lists))
    return out


@pytest.mark.parametrize("first_id", rw.FIRST_IDS)
def test_rows_hand_made_lists(ctx, hand_made, first_id):
    import folddisco_amd as fd
    lists, (v, h, o) = hand_made[first_id]
    ix = fd.FolddiscoIndex.load(ctx, h, o, v, rw.N, first_id=first_id)
    for lo, hi in rw.WINDOWS:
        a, b = first_id + lo, first_id + hi
        want = rw.expected_rows(lists, h, a, b)
        got = ix.rows(a, b)
        assert _eq(got, want), (lo, hi)
        assert _eq(indexio.rows_host(v, h, o, rw.N, first_id=first_id, lo=a, hi=b, threads=2), want), (lo, hi)
        assert len(got[1]) == hi - lo + 1
    assert _eq(ix.rows(first_id + rw.B, first_id + rw.B + 256), ix.rows(first_id + rw.B, first_id + rw.B + 256))      # the same bytes from run to run
    assert all(np.array_equal(x, y) for x, y in zip(ix.export(), (v, h, o)))                                          # the index is not changed


def test_rows_empty_index(ctx):
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.load(ctx, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint8), 10, first_id=3)
    h, off = ix.rows()
    assert len(h) == 0 and h.dtype == np.uint32 and off.tolist() == [0] * 11 and off.dtype == np.uint64


# ---- 2. against the hasher: the test that pins the meaning
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


@pytest.fixture(scope="module")
def hasher(ctx, synth180):
    """the sorted-unique hashes of every structure from the batch hasher, once"""
    import folddisco_amd as fd
    h, off = fd.get_geometric_hash_as_u32(ctx, ctx.upload(synth180), sort_dedup=True)
    assert len(h) > 100000
    return h, off


def _build(ctx, items, lo, hi, first_id):
    import folddisco_amd as fd
    return fd.FolddiscoIndex.build(ctx, ctx.upload(fd.PackedStructures.concat(items[lo:hi])), first_id=first_id)


def _check_windows(ix, want, first_id):
    assert _eq(ix.rows(), want)
    for lo, hi in WINDOWS:
        assert _eq(ix.rows(first_id + lo, first_id + hi), _cut(want, lo, hi)), (first_id, lo, hi)


@pytest.mark.parametrize("first_id", [0, 16300])
def test_rows_equal_the_hasher(ctx, items, hasher, first_id):
    import folddisco_amd as fd
    built = _build(ctx, items, 0, N, first_id)
    _check_windows(built, hasher, first_id)
    v, h, o = built.export()
    loaded = fd.FolddiscoIndex.load(ctx, h, o, v, N, first_id=first_id)      # no last ids
    _check_windows(loaded, hasher, first_id)
    assert _eq(indexio.rows_host(v, h, o, N, first_id=first_id, threads=3), hasher)
    halves = [_build(ctx, items, 0, 77, first_id), _build(ctx, items, 77, N, first_id + 77)]
    _check_windows(fd.FolddiscoIndexSet(halves).merge(), hasher, first_id)
    # the other index operations, each against the hasher's rows under the same selection, permutation or shift: no second build
    keep = np.ones(N, bool)
    keep[[0, 5, 57, 58, 100, N - 1]] = False
    kept = np.nonzero(keep)[0]
    pruned = loaded.remove(keep)
    assert _eq(pruned.rows(), _select(hasher, kept))
    assert _eq(pruned.rows(first_id + 13, first_id + 141), _select(hasher, kept[13:141]))
    new_id = np.random.Generator(np.random.PCG64(5)).permutation(N).astype(np.uint32)
    moved = built.permute(new_id)
    _check_windows(moved, _select(hasher, np.argsort(new_id)), first_id)
    shifted = built.rebase(first_id + 2097100)
    _check_windows(shifted, hasher, first_id + 2097100)


def test_rows_of_a_multiple_bins_build(ctx, synth180):
    """no hasher serves it: the rows equal the NumPy transposition of the exported lists"""
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth180), multiple_bins=[(16, 4), (8, 3)])
    v, h, o = ix.export()
    term = np.nonzero(v < 128)[0]                                            # a posting ends at every byte without the continuation bit
    lst = np.searchsorted(o, term, side="right") - 1                         # its list
    # decode: value of every varint, then running sums per list
    start = np.concatenate([[0], term[:-1] + 1])
    val = np.zeros(len(term), np.uint64)
    for b in range(5):
        p = start + b
        inside = p <= term
        val[inside] |= (v[p[inside]].astype(np.uint64) & np.uint64(0x7f)) << np.uint64(7 * b)
    run = np.cumsum(val)
    first = np.searchsorted(term, o[:-1])                                    # first posting of every list
    before = np.concatenate([[0], run])[first]
    sid = (run - before[lst]).astype(np.int64)
    assert sid.min() >= 0 and sid.max() < N and len(sid) == ix.num_postings
    order = np.argsort(sid, kind="stable")
    want = (h[lst][order].astype(np.uint32), np.searchsorted(sid[order], np.arange(N + 1)).astype(np.uint64))
    assert _eq(ix.rows(), want)
    assert _eq(ix.rows(13, 141), _cut(want, 13, 141))


# ---- 3. refusals: both outputs NULL, the context usable afterwards
def _raw(ctx, ix, lo, hi):
    hp, op = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)()
    hp.contents, op.contents = C.c_uint32(1), C.c_uint64(1)                  # not NULL on entry
    rc = ctx.L.fdgpu_index_rows(ctx.h, ix.h, lo, hi, C.byref(hp), C.byref(op))
    return rc, bool(hp), bool(op)


def test_rows_errors(ctx):
    import folddisco_amd as fd
    load = lambda lists, off=None: fd.FolddiscoIndex.load(ctx, rw.pack(lists)[1], rw.pack(lists)[2] if off is None else off, rw.pack(lists)[0], 1000, first_id=100)
    good_lists = [[100, 105], [101, 300], [120]]
    good = load(good_lists)
    want = indexio.rows_host(*rw.pack(good_lists), 1000, first_id=100)
    assert _eq(good.rows(), want)
    for lo, hi in ((99, 200), (100, 1101), (200, 150)):                      # a window past the index, or backwards
        assert _raw(ctx, good, lo, hi) == (-1, False, False)
        assert _eq(good.rows(), want)
    for lists in ([[100, 105], [101, 1100], [120]], [[100, 105], [99, 300], [120]]):      # one id outside [first_id, first_id + n)
        assert _raw(ctx, load(lists), 100, 400) == (-1, False, False)
        with pytest.raises(ValueError, match=r"\(-1\)"):
            indexio.rows_host(*rw.pack(lists), 1000, first_id=100, lo=100, hi=400)
        assert _eq(good.rows(), want)
    o = rw.pack(good_lists)[2]
    bad = o.copy()
    bad[1], bad[2] = o[2], o[1]                                              # offsets that do not ascend
    assert _raw(ctx, load(good_lists, bad), 100, 1100) == (-1, False, False)
    with pytest.raises(fd.FdgpuError):
        load(good_lists, bad).rows()
    assert _eq(good.rows(), want) and _eq(good.rows(100, 121), _cut(want, 0, 21))


# ---- 4. the commands
def _cli(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


@pytest.fixture(scope="module")
def ser_index(tmp_path_factory):
    root = tmp_path_factory.mktemp("rows_cli")
    d = os.path.join(str(root), "db")
    os.makedirs(d)
    for p in SER:
        shutil.copy(p, os.path.join(d, os.path.basename(p)))
    prefix = os.path.join(str(root), "ix")
    assert _cli(["index", "-p", d, "-i", prefix, "--coords"]) == 0
    return root, prefix


def test_cli_rows_device_equals_host(ser_index, tmp_path, capsys):
    _, prefix = ser_index
    dev, host = str(tmp_path / "dev.npz"), str(tmp_path / "host.npz")
    capsys.readouterr()
    assert _cli(["rows", "-i", prefix, "-o", dev, "--window", "2", "--verify"]) == 0
    line = capsys.readouterr().out
    assert _cli(["rows", "-i", prefix, "-o", host, "--host", "-t", "2"]) == 0
    a, b = np.load(dev), np.load(host)
    assert sorted(a.files) == ["hashes", "ids", "row_off", "tids"] and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a.files)
    n, longest = len(a["hashes"]), int(np.diff(a["row_off"].astype(np.int64)).max())
    assert line == f"[OK] {dev}: 5 structures, {n} hashes, longest row {longest}\n" and n > 10000
    tids = a["tids"].tolist()
    (tmp_path / "t.txt").write_text(f"{tids[3]}\n{tids[0]}\n{tids[4]}\n")
    assert _cli(["rows", "-i", prefix, "-o", dev, "--tids", str(tmp_path / "t.txt")]) == 0
    c = np.load(dev)
    assert c["ids"].tolist() == [3, 0, 4] and c["tids"].tolist() == [tids[3], tids[0], tids[4]]
    assert _eq((c["hashes"], c["row_off"]), _select((a["hashes"], a["row_off"]), [3, 0, 4]))
    (tmp_path / "t.txt").write_text(f"{tids[3]}\nnot-a-tid\n")
    assert _cli(["rows", "-i", prefix, "-o", dev, "--tids", str(tmp_path / "t.txt")]) == 1
    assert _cli(["rows", "-i", str(tmp_path / "nope"), "-o", dev]) == 2


def test_cli_verify_structures(ser_index, tmp_path, capsys):
    root, prefix = ser_index
    capsys.readouterr()
    assert _cli(["verify", "-i", prefix]) == 0
    plain = capsys.readouterr().out
    assert _cli(["verify", "-i", prefix, "--structures", "--window", "2"]) == 0
    out = capsys.readouterr().out
    assert out.startswith(plain) and len(out.splitlines()) == len(plain.splitlines()) + 1                 # one more [OK] line, the rest as before
    last = out.splitlines()[-1]
    assert last.startswith(f"[OK] {prefix}: the index describes the coordinates of {prefix}.coords: 5 structures, ") and last.endswith(" hashes compared")
    # the same stamp, one structure's C-alpha coordinates displaced by 3 A
    st = indexio.CoordStore.open(prefix + ".coords")
    moved = str(tmp_path / "moved.coords")
    pieces = []
    for s in range(st.n_struct):
        a = st.slice(s, s + 1)
        if s == 2:
            a.ps.ca_xyz = (np.asarray(a.ps.ca_xyz) + np.float32(3.0)).astype(np.float32)
        pieces.append(a)
    indexio.write_coords(moved, pieces, st.stamp)
    tids = [r.split("\t")[1] for r in indexio.read_lookup_rows(prefix + ".lookup")]
    assert _cli(["verify", "-i", prefix, "--structures", "--coords", moved]) == 1
    out = capsys.readouterr().out
    fail = [l for l in out.splitlines() if l.startswith("[FAIL]")]
    assert len(fail) == 1 and fail[0].startswith(f"[FAIL] structure 2 {tids[2]}: index row ") and "coordinates" in fail[0]
    # the gap this closes: the plain verify and the stamp check still pass with that store beside the index
    other = str(tmp_path / "ix2")
    for ext in ("", ".offset", ".lookup", ".type"):
        shutil.copy(prefix + ext, other + ext)
    shutil.copy(moved, other + ".coords")
    assert _cli(["verify", "-i", other]) == 0 and "stamp matches the index files" in capsys.readouterr().out
    assert _cli(["verify", "-i", other, "--structures"]) == 1
    assert f"[FAIL] structure 2 {tids[2]}" in capsys.readouterr().out
