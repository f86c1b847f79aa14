"""Signature clusters on the device (fdgpu_signature_clusters, Context.signature_clusters, `python -m folddisco_amd cluster`): the device result
equals the host form and an independent brute force byte for byte on the hand-made tables for every size, threshold and walk order, on the
extreme tables and the planted cases, and under every split of the representatives over workgroups; two runs, the refusals, the closing
property through the pairs call, the command on the device against --host, and `cluster --redundant` followed by `update --remove`."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

from folddisco_amd import indexio
from tests import cluster_cases as cc
from tests.helpers import SER

pytestmark = pytest.mark.gpu

DT = indexio.SIGNATURE_NEIGHBOR_DTYPE
SDT = indexio.SIGNATURE_DTYPE


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def table(n):
    return cc.table(n, SDT)


@pytest.mark.parametrize("n", cc.SIZES)
def test_device_equals_host_and_brute_force(ctx, n):
    S = table(n)
    for thr in cc.THRESHOLDS:
        for name in cc.ORDERS:
            order = cc.order_of(S, name)
            host = indexio.signature_clusters_host(S, order, thr64=thr, threads=2)
            got = ctx.signature_clusters(S, order, thr64=thr)
            assert got.dtype == DT and got.shape == (n,) and got.tobytes() == host.tobytes(), (n, thr, name)
        assert ctx.signature_clusters(S, thr64=thr).tobytes() == indexio.signature_clusters_host(S, thr64=thr).tobytes()      # no order: position order
    order = cc.order_of(S, "random")
    want = cc.brute_clusters(S, order, 48, DT)
    got = ctx.signature_clusters(S, order, min_similarity=0.75)
    assert all(np.array_equal(got[f], want[f]) for f in DT.names)


def test_extreme_tables_and_planted_cases(ctx):
    R = cc.all_random(SDT)
    ids = np.arange(len(R))
    for thr in (1, 64):
        got = ctx.signature_clusters(R, thr64=thr)
        assert np.array_equal(got["id"], ids) and got.tobytes() == indexio.signature_clusters_host(R, thr64=thr).tobytes()
    K = cc.all_copies(SDT)
    got = ctx.signature_clusters(K, np.roll(ids, -123).astype(np.uint32), thr64=64)
    assert (got["id"] == 123).all() and (got["match"] == 64).all() and (got["flags"] == 1).all()
    for name, S, order, thr, expect in cc.planted(SDT):
        got = ctx.signature_clusters(S, order, thr64=thr)
        assert {p: int(got["id"][p]) for p in expect} == expect, name
        assert got.tobytes() == indexio.signature_clusters_host(S, order, thr64=thr).tobytes(), name


@pytest.mark.parametrize("n", cc.SPLIT_SIZES)
def test_every_split_gives_the_same_bytes(ctx, n, monkeypatch):
    tabs = [(table(n), cc.order_of(table(n), "random"), 48)]
    if n == 700:
        tabs.append((cc.all_random(SDT), None, 32))                            # eleven tiles of representatives: every split below has a merge
    for S, order, thr in tabs:
        monkeypatch.delenv("FDGPU_SG_CL_SPLIT", raising=False)
        base = ctx.signature_clusters(S, order, thr64=thr).tobytes()
        assert base == indexio.signature_clusters_host(S, order, thr64=thr).tobytes()
        for split in cc.SPLITS:
            monkeypatch.setenv("FDGPU_SG_CL_SPLIT", str(split))               # read per call
            assert ctx.signature_clusters(S, order, thr64=thr).tobytes() == base, (n, split)
    monkeypatch.delenv("FDGPU_SG_CL_SPLIT", raising=False)
    assert ctx.signature_clusters(S, order, thr64=thr).tobytes() == base       # two runs give the same bytes


def test_refusals_launch_nothing(ctx):
    import folddisco_amd as fd
    S = table(65)
    good = np.arange(65, dtype=np.uint32)
    ctx.enable_timing(True)
    ok = ctx.signature_clusters(table(257), thr64=32)
    stages = [s for s, _, _ in ctx.last_timings()]
    assert stages == ["sigcl_upload", "sigcl_resolve", "sigcl_scan", "sigcl_resolve", "sigcl_copy"]      # two blocks; nothing to scan before the first
    twice, beyond = good.copy(), good.copy()
    twice[7] = 8
    beyond[64] = 65
    s = S.ctypes.data
    for args in ((s, 65, None, 0), (s, 65, None, 65), (s, 1 << 32, None, 32), (None, 3, None, 32), (s, 65, twice.ctypes.data, 32), (s, 65, beyond.ctypes.data, 32),
                 (s, 64, good[1:].copy().ctypes.data, 32)):
        out = C.c_void_p(1)
        assert ctx.L.fdgpu_signature_clusters(ctx.h, *args, C.byref(out)) == -1 and not out, args[1:]
        assert ctx.L.fdgpu_last_error(ctx.h).decode().startswith("signature clusters:")
    for kw in (dict(thr64=0), dict(thr64=65)):
        with pytest.raises(fd.FdgpuError, match="signature clusters:"):
            ctx.signature_clusters(S, **kw)
    with pytest.raises(ValueError, match="^signature clusters:"):
        ctx.signature_clusters(S, good[:5])
    assert [s for s, _, _ in ctx.last_timings()] == stages                   # the refused calls recorded no stage: nothing was launched
    ctx.enable_timing(False)
    assert ctx.signature_clusters(S[:0]).shape == (0,)
    assert ctx.signature_clusters(table(257), thr64=32).tobytes() == ok.tobytes()      # the context is usable afterwards


@pytest.mark.parametrize("thr", (32, 48))
def test_no_two_representatives_are_a_reported_pair(ctx, thr):
    S = table(700)
    order = cc.order_of(S, "n_descending")
    got = ctx.signature_clusters(S, order, thr64=thr)
    ids = np.arange(len(S))
    reps = ids[got["id"] == ids]
    assert 64 < len(reps) < len(S)
    assert len(ctx.signature_pairs(S[reps], thr64=thr)) == 0
    assert len(ctx.signature_pairs(S[reps], thr64=thr - 8)) > 0               # the pairs call does see pairs just below the threshold


def _cli(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


def test_cli_cluster_then_remove_leaves_no_duplicates(tmp_path, capsys):
    """the serine peptidase index joined with a copy of itself under other tids: every copy joins its original; after `update --remove` of the
    members `dups` reports nothing"""
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
    dev, host, red, red_h = (str(tmp_path / f) for f in ("dev.tsv", "host.tsv", "red.txt", "red_host.txt"))
    capsys.readouterr()
    assert _cli(["cluster", "-i", joined, "-o", dev, "--redundant", red, "--window", "3", "--verify", "--confirm", "--rep-by", "id"]) == 0
    line = capsys.readouterr().out
    assert _cli(["cluster", "-i", joined, "-o", host, "--redundant", red_h, "--host", "-t", "2", "--confirm", "--rep-by", "id"]) == 0
    assert capsys.readouterr().out == line
    text = open(dev).read()
    assert text == open(host).read() and open(red).read() == open(red_h).read()
    rows = [l.split("\t") for l in text.splitlines()]
    assert [(int(c[0]), int(c[3])) for c in rows] == sorted((int(c[0]), int(c[3])) for c in rows)      # by (rep_id, id)
    copies = {int(c[3]): c for c in rows if int(c[3]) >= S}
    assert len(copies) == S and all(c[9] == "identical" and c[10] == "1.0000" and int(c[0]) < S for c in copies.values())
    n_rep = sum(c[9] == "representative" for c in rows)
    n_mem = len(rows) - n_rep
    assert f"[OK] {joined}: {2 * S} structures, {n_rep} clusters (" in line and f"), {n_mem} members (" in line and line.endswith(", threshold 58/64\n")
    members = open(red).read().splitlines()
    assert len(members) == n_mem >= S
    # the other walks agree with the host form too
    for by in ("hashes", "nres", "plddt"):
        assert _cli(["cluster", "-i", joined, "-o", dev, "--rep-by", by, "--min-similarity", "0.5"]) == 0
        assert _cli(["cluster", "-i", joined, "-o", host, "--rep-by", by, "--min-similarity", "0.5", "--host"]) == 0
        assert open(dev).read() == open(host).read()
    # what the list is for
    out = str(tmp_path / "nr")
    assert _cli(["update", "-i", joined, "--remove", red, "-o", out]) == 0
    capsys.readouterr()
    assert _cli(["dups", "-i", out, "-o", str(tmp_path / "dups.tsv")]) == 0
    msg = capsys.readouterr().out
    unclustered = 2 * S - len(rows)
    assert f"{n_rep + unclustered} structures, 0 pairs" in msg and open(str(tmp_path / "dups.tsv")).read() == ""
    assert _cli(["cluster", "-i", joined, "-o", dev, "--min-similarity", "0"]) == 1
    assert _cli(["cluster", "-i", joined, "-o", dev, "--rep-by", "size"]) == 1
    assert _cli(["cluster", "-i", str(tmp_path / "nope"), "-o", dev]) == 2
    assert not [f for f in os.listdir(tmp_path) if "cluster-tmp" in f]
