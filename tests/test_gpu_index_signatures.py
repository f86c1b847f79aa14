"""Index signatures on the device (fdgpu_index_signatures, FolddiscoIndex.signatures, fdgpu_signature_pairs, `python -m folddisco_amd dups`):
the table of hand-made rows equals the host form and a pure-Python statement of the definition at every window, the signatures of a built
index equal the reduction of what the batch hasher gives and move with their structures under permute, rebase, split and merge, and the
device compare equals the host form record for record."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from folddisco_amd import indexio
from tests import signature_cases as sc
from tests.helpers import SER, oracle_structs_to_packed

pytestmark = pytest.mark.gpu

N = 180
PAIR_FIELDS = list(indexio.SIGNATURE_PAIR_DTYPE.names)


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


def _same(a, b):
    return a.dtype == b.dtype == indexio.SIGNATURE_DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. hand-made rows, independent of the GPU build: device == host == Python at every window
@pytest.fixture(scope="module")
def want():
    return sc.table_of(sc.ROWS, indexio.SIGNATURE_DTYPE)


@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_signatures_hand_made_rows(ctx, want, first_id):
    import folddisco_amd as fd
    v, h, o, _ = sc.index(first_id)
    ix = fd.FolddiscoIndex.load(ctx, h, o, v, sc.N, first_id=first_id)
    assert _same(indexio.signatures_host(v, h, o, sc.N, first_id=first_id, threads=2), want)
    for window in sc.WINDOWS:
        got = ix.signatures(window=window)
        assert _same(got, want), window
        assert got.tobytes() == ix.signatures(window=window).tobytes()                                  # the same bytes from run to run
    assert _same(ix.signatures(), want) and _same(ix.signatures(window=0), want)                         # the default window, by either spelling
    for lo, hi in sc.RANGES:
        assert _same(ix.signatures(first_id + lo, first_id + hi, window=257), want[lo:hi]), (lo, hi)
    assert all(np.array_equal(x, y) for x, y in zip(ix.export(), (v, h, o)))                             # the index is not changed


def test_signatures_empty_index(ctx):
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.load(ctx, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint8), 10, first_id=3)
    got = ix.signatures()
    assert got.dtype == indexio.SIGNATURE_DTYPE and len(got) == 10
    assert (got["n"] == 0).all() and (got["d0"] == 0).all() and (got["d1"] == 0).all() and (got["sk"] == sc.EMPTY).all() and (got["reserved"] == 0).all()
    assert len(ix.signatures(5, 5)) == 0


# ---- 2. against the hasher
def test_signatures_of_the_golden_structures_equal_the_hasher(ctx):
    import folddisco_amd as fd
    import oracle
    ps, _ = oracle_structs_to_packed([oracle.read_pdb(p) for p in SER])
    batch = ctx.upload(ps)
    ix = fd.FolddiscoIndex.build(ctx, batch)
    h, off = fd.get_geometric_hash_as_u32(ctx, batch, sort_dedup=True)
    want = indexio.signatures_from_rows(h, off)
    assert len(h) > 10000 and (want["n"] > 0).all()
    assert _same(ix.signatures(), want) and _same(ix.signatures(window=2), want)
    v, hh, o = ix.export()
    assert _same(indexio.signatures_host(v, hh, o, len(SER), threads=2), want)


@pytest.fixture(scope="module")
def built(ctx):
    import folddisco_amd as fd
    from folddisco_amd import synth
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(synth.to_packed(synth.generate(N, seed=31))))
    return ix, np.array(ix.signatures())


def test_signatures_move_with_their_structures(ctx, built):
    import folddisco_amd as fd
    ix, sig = built
    assert (sig["n"] > 100).all() and _same(sig, indexio.signatures_from_rows(*ix.rows()))
    p = np.random.Generator(np.random.PCG64(5)).permutation(N).astype(np.uint32)
    moved = ix.permute(p).signatures(window=64)
    assert _same(moved[p], sig)                                               # permute(p).signatures()[p[s]] == signatures()[s]
    assert _same(ix.rebase(2097100).signatures(window=50), sig)
    parts = ix.split([0, 77, N])
    assert _same(np.concatenate([q.signatures() for q in parts]), sig)
    assert _same(fd.FolddiscoIndexSet(parts).merge().signatures(), sig)
    keep = np.ones(N, bool)
    keep[[0, 5, 57, N - 1]] = False
    assert _same(ix.remove(keep).signatures(), sig[keep])


# ---- 3. the compare: device == host on the hand-made tables
@pytest.fixture(scope="module")
def tables():
    return {n: sc.pair_table(n, 100 + n, indexio.SIGNATURE_DTYPE) for n in sc.PAIR_SIZES}


@pytest.mark.parametrize("n", sc.PAIR_SIZES)
def test_signature_pairs_device_equals_host(ctx, tables, n):
    A = tables[n]
    for B in (None, sc.other_table(A, 7)):
        for thr in sc.THRESHOLDS:
            host = indexio.signature_pairs_host(A, B, thr64=thr, threads=2)
            got = ctx.signature_pairs(A, B, thr64=thr)
            assert got.dtype == host.dtype and got.tobytes() == host.tobytes(), (n, B is None, thr)
            key = got["a"].astype(np.int64) << 32 | got["b"].astype(np.int64)
            assert (np.diff(key) > 0).all()                                   # sorted by (a, b), no pair twice
            if B is None:
                assert (got["a"] < got["b"]).all()
    want = sc.brute_pairs(A, None, 48, indexio.SIGNATURE_PAIR_DTYPE)
    got = ctx.signature_pairs(A, min_similarity=0.75)
    assert all(np.array_equal(got[k], want[k]) for k in PAIR_FIELDS)


def test_signature_pairs_device_cap(ctx, tables):
    A = tables[129]
    for B in (None, sc.other_table(A, 7)):
        true = len(sc.brute_pairs(A, B, 1, indexio.SIGNATURE_PAIR_DTYPE))
        assert true > 1000 and len(ctx.signature_pairs(A, B, thr64=1, max_pairs=true)) == true          # the cap itself fits
        with pytest.raises(indexio.SignaturePairsOverflow) as e:
            ctx.signature_pairs(A, B, thr64=1, max_pairs=true - 1)
        assert e.value.count == true
        assert ctx.signature_pairs(A, B, thr64=1).tobytes() == indexio.signature_pairs_host(A, B, thr64=1).tobytes()      # the context is usable afterwards
    assert len(ctx.signature_pairs(A[:0], thr64=1)) == 0 and len(ctx.signature_pairs(A, A[:0], thr64=1)) == 0


# ---- 4. argument refusals: EINVAL with a message, the outputs NULL, nothing launched
def test_signature_argument_refusals(ctx, tables):
    import folddisco_amd as fd
    from tests.rebase_cases import pack
    v, h, o = pack([[100, 105], [101, 300], [120]])
    ix = fd.FolddiscoIndex.load(ctx, h, o, v, 1000, first_id=100)
    good = np.array(ix.signatures())
    assert good["n"].sum() == 5
    ctx.enable_timing(True)
    for lo, hi in ((99, 200), (100, 1101), (200, 150)):                      # a range past the index, or backwards
        out = C.c_void_p(1)
        assert ctx.L.fdgpu_index_signatures(ctx.h, ix.h, lo, hi, 0, C.byref(out)) == -1 and not out
        assert ctx.L.fdgpu_last_error(ctx.h).decode().startswith("index signatures:")
        with pytest.raises(fd.FdgpuError, match="index signatures:"):
            ix.signatures(lo, hi)
    A = tables[65]
    assert len(ctx.signature_pairs(A, thr64=48)) > 0
    stages = [s for s, _, _ in ctx.last_timings()]
    assert "sigpairs_match" in stages
    for thr in (0, 65):
        pp, n = C.c_void_p(1), C.c_uint64(7)
        assert ctx.L.fdgpu_signature_pairs(ctx.h, A.ctypes.data, len(A), None, 0, thr, 1 << 20, C.byref(pp), C.byref(n)) == -1 and not pp and n.value == 0
        assert "thr64" in ctx.L.fdgpu_last_error(ctx.h).decode()
        with pytest.raises(fd.FdgpuError, match="thr64"):
            ctx.signature_pairs(A, thr64=thr)
    assert [s for s, _, _ in ctx.last_timings()] == stages                   # the refused calls recorded no stage: nothing was launched
    ctx.enable_timing(False)
    assert _same(np.array(ix.signatures()), good)


# ---- 5. the command
def _cli(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


def test_cli_dups_device_equals_host(tmp_path, capsys):
    """the serine peptidase index joined with a copy of itself under other tids: every structure pairs with its copy as identical"""
    prefixes = []
    for name in ("db", "mirror"):
        d = str(tmp_path / name)
        os.makedirs(d)
        for p in SER:
            shutil.copy(p, os.path.join(d, ("" if name == "db" else "m_") + os.path.basename(p)))
        prefixes.append(str(tmp_path / f"ix_{name}"))
        assert _cli(["index", "-p", d, "-i", prefixes[-1]]) == 0
    joined = str(tmp_path / "joined")
    assert _cli(["merge", "-i", *prefixes, "-o", joined]) == 0
    S = len(SER)
    dev, host = str(tmp_path / "dev.tsv"), str(tmp_path / "host.tsv")
    capsys.readouterr()
    assert _cli(["dups", "-i", joined, "-o", dev, "--window", "3", "--verify", "--confirm"]) == 0
    line = capsys.readouterr().out
    assert _cli(["dups", "-i", joined, "-o", host, "--host", "-t", "2", "--confirm"]) == 0
    assert capsys.readouterr().out == line
    text = open(dev).read()
    assert text == open(host).read()
    rows = [l.split("\t") for l in text.splitlines()]
    ident = [(int(c[0]), int(c[3])) for c in rows if c[9] == "identical"]
    assert ident == [(s, s + S) for s in range(S)] and all(c[6] == c[7] and c[8] == c[10] == "1.0000" for c in rows if c[9] == "identical")
    assert all(os.path.basename(c[4]) == "m_" + os.path.basename(c[1]) for c in rows if c[9] == "identical")
    assert line == f"[OK] {joined}: {2 * S} structures, {len(rows)} pairs ({S} identical), threshold 58/64\n"
    # --against: the mirror against the database, only the identical ones
    assert _cli(["dups", "-i", prefixes[1], "--against", prefixes[0], "-o", dev, "--identical-only"]) == 0
    assert _cli(["dups", "-i", prefixes[1], "--against", prefixes[0], "-o", host, "--identical-only", "--host"]) == 0
    text = open(dev).read()
    assert text == open(host).read() and [(int(l.split("\t")[0]), int(l.split("\t")[3])) for l in text.splitlines()] == [(s, s) for s in range(S)]
    assert capsys.readouterr().out.count(f"{S} x {S} structures, {S} pairs ({S} identical), threshold 64/64") == 2
