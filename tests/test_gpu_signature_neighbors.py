"""Signature neighbours on the device (fdgpu_signature_neighbors, Context.signature_neighbors, `python -m folddisco_amd neighbors`): the device
result equals the host form byte for byte on the hand-made tables for every size, k and threshold, inside one table and between two, and
under every split of the candidates over workgroups; the exclusion, empty tables, the refusals, and the command on the device against --host."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from folddisco_amd import indexio
from tests import neighbor_cases as nc
from tests.helpers import SER

pytestmark = pytest.mark.gpu

DT = indexio.SIGNATURE_NEIGHBOR_DTYPE


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables():
    out = {}
    for n in nc.SIZES:
        A = nc.table(n, indexio.SIGNATURE_DTYPE)
        out[n] = (A, nc.other(A))
    return out


@pytest.mark.parametrize("n", nc.SIZES)
def test_device_equals_host(ctx, tables, n):
    A, B = tables[n]
    for Q, D in ((A, None), (B, A)):
        for k in nc.KS:
            for thr in nc.THRESHOLDS:
                host = indexio.signature_neighbors_host(Q, D, k=k, thr64=thr, threads=2)
                got = ctx.signature_neighbors(Q, D, k=k, thr64=thr)
                assert got.dtype == DT and got.shape == (len(Q), k) and got.tobytes() == host.tobytes(), (n, D is None, k, thr)
    want = nc.brute_neighbors(A, None, 4, 32, None, DT)                      # one spot check against the numpy brute force
    got = ctx.signature_neighbors(A, k=4, min_similarity=0.5)
    assert all(np.array_equal(got[f], want[f]) for f in DT.names)


@pytest.mark.parametrize("n", (129, 600))
def test_every_split_gives_the_same_bytes(ctx, tables, n, monkeypatch):
    A, B = tables[n]
    ctx.enable_timing(True)
    try:
        for Q, D in ((A, None), (B, A)):
            tiles = (len(A) + 63) // 64
            for k in nc.KS:
                monkeypatch.delenv("FDGPU_SG_NB_SPLIT", raising=False)
                base = ctx.signature_neighbors(Q, D, k=k, thr64=1).tobytes()
                assert base == indexio.signature_neighbors_host(Q, D, k=k, thr64=1).tobytes()
                for split in nc.SPLITS:
                    monkeypatch.setenv("FDGPU_SG_NB_SPLIT", str(split))       # read per call
                    assert ctx.signature_neighbors(Q, D, k=k, thr64=1).tobytes() == base, (n, D is None, k, split)
                    stages = [s for s, _, _ in ctx.last_timings()]
                    assert ("signb_merge" in stages) == (min(split, tiles, 64) > 1) and "signb_scan" in stages, (split, stages)
    finally:
        ctx.enable_timing(False)


def test_exclude_and_empty_tables(ctx, tables):
    A, _ = tables[257]
    ids = np.array([0, 8, 9, 63, 64, 200, 256, 8], np.uint32)
    for k in nc.KS:
        got = ctx.signature_neighbors(A[ids], A, k=k, thr64=1, exclude=ids)
        assert got.tobytes() == ctx.signature_neighbors(A, k=k, thr64=1)[ids].tobytes()
        assert got.tobytes() == indexio.signature_neighbors_host(A[ids], A, k=k, thr64=1, exclude=ids).tobytes()
    free = ctx.signature_neighbors(A[ids], A, k=1)
    assert free["id"][0, 0] == 0 and free["flags"][0, 0] == 1                # nothing excluded: record 0 finds itself
    assert ctx.signature_neighbors(A[:0], A, k=4).shape == (0, 4) and ctx.signature_neighbors(A[:0], k=4).shape == (0, 4)
    none = ctx.signature_neighbors(A, A[:0], k=4)
    assert none.tobytes() == indexio.signature_neighbors_host(A, A[:0], k=4).tobytes() and (none["id"] == nc.NO_ID).all()
    few = ctx.signature_neighbors(A[:5], k=32)                                # k greater than nD
    assert few.tobytes() == indexio.signature_neighbors_host(A[:5], k=32).tobytes() and (few["id"][:, 4:] == nc.NO_ID).all()


def test_refusals_launch_nothing(ctx, tables):
    import folddisco_amd as fd
    A, B = tables[65]
    ctx.enable_timing(True)
    good = ctx.signature_neighbors(B, A, k=4, thr64=32)
    stages = [s for s, _, _ in ctx.last_timings()]
    assert "signb_scan" in stages and "signb_upload" in stages and "signb_copy" in stages
    x = np.zeros(len(B), np.uint32)
    a, b = A.ctypes.data, B.ctypes.data
    for args in ((b, len(B), a, len(A), None, 0, 1), (b, len(B), a, len(A), None, 33, 1), (b, len(B), a, len(A), None, 8, 0), (b, len(B), a, len(A), None, 8, 65),
                 (b, 1 << 32, a, len(A), None, 8, 1), (b, len(B), a, 1 << 32, None, 8, 1), (a, len(A), None, 0, x.ctypes.data, 8, 1), (None, 3, a, len(A), None, 8, 1)):
        out = C.c_void_p(1)
        assert ctx.L.fdgpu_signature_neighbors(ctx.h, *args, C.byref(out)) == -1 and not out, args[1:]
        assert ctx.L.fdgpu_last_error(ctx.h).decode().startswith("signature neighbors:")
    for kw in (dict(k=0), dict(k=33), dict(thr64=0), dict(thr64=65), dict(exclude=np.zeros(len(A), np.uint32))):
        with pytest.raises(fd.FdgpuError, match="signature neighbors:"):
            ctx.signature_neighbors(A, **kw)
    assert [s for s, _, _ in ctx.last_timings()] == stages                   # the refused calls recorded no stage: nothing was launched
    ctx.enable_timing(False)
    assert ctx.signature_neighbors(B, A, k=4, thr64=32).tobytes() == good.tobytes()      # the context is usable afterwards


def _cli(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


def test_cli_neighbors_device_equals_host(tmp_path, capsys):
    """the serine peptidase index joined with a copy of itself under other tids: every structure's nearest neighbour is its copy"""
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
    assert _cli(["neighbors", "-i", joined, "-k", "3", "-o", dev, "--window", "3", "--verify", "--confirm"]) == 0
    line = capsys.readouterr().out
    assert _cli(["neighbors", "-i", joined, "-k", "3", "-o", host, "--host", "-t", "2", "--confirm"]) == 0
    assert capsys.readouterr().out == line
    text = open(dev).read()
    assert text == open(host).read()
    rows = [l.split("\t") for l in text.splitlines()]
    assert [(int(c[0]), int(c[3])) for c in rows] == sorted((int(c[0]), int(c[3])) for c in rows)      # by (id, rank)
    first = [c for c in rows if c[3] == "1"]
    assert [(int(c[0]), int(c[4])) for c in first] == [(s, (s + S) % (2 * S)) for s in range(2 * S)]
    assert all(c[10] == "identical" and c[9] == c[11] == "1.0000" and c[7] == c[8] and c[2] == c[6] for c in first)
    assert all(os.path.basename(c[5]) == "m_" + os.path.basename(c[1]) for c in first[:S])
    assert line == f"[OK] {joined}: {2 * S} structures, k = 3, {len(rows)} rows, 0 without a neighbour, {2 * S} with an identical nearest, floor 1/64\n"
    # --against: the mirror against the database, the nearest only
    assert _cli(["neighbors", "-i", prefixes[1], "--against", prefixes[0], "-k", "1", "-o", dev]) == 0
    assert _cli(["neighbors", "-i", prefixes[1], "--against", prefixes[0], "-k", "1", "-o", host, "--host"]) == 0
    text = open(dev).read()
    assert text == open(host).read()
    assert [(int(l.split("\t")[0]), int(l.split("\t")[4]), l.split("\t")[10]) for l in text.splitlines()] == [(s, s, "identical") for s in range(S)]
    assert capsys.readouterr().out.count(f"{S} x {S} structures, k = 1, {S} rows, 0 without a neighbour, {S} with an identical nearest, floor 1/64") == 2
    # --tids: only their rows, the same as in the full run
    all_tids = [l.split("\t")[1] for l in open(joined + ".lookup").read().splitlines()]
    pick = [S + 1, 2]
    with open(tmp_path / "tids.txt", "w") as f:
        f.write("".join(all_tids[s] + "\n" for s in pick))
    part = str(tmp_path / "part.tsv")
    assert _cli(["neighbors", "-i", joined, "-k", "3", "-o", part, "--tids", str(tmp_path / "tids.txt"), "--confirm"]) == 0
    assert open(part).read() == "".join("\t".join(c) + "\n" for c in rows if int(c[0]) in pick) and open(part).read()
    assert _cli(["neighbors", "-i", joined, "-o", part, "--min-similarity", "0"]) == 1
    assert _cli(["neighbors", "-i", str(tmp_path / "nope"), "-o", part]) == 2
    assert not [f for f in os.listdir(tmp_path) if "neighbors-tmp" in f]
