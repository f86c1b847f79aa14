"""Seeded signature clusters on the device (fdgpu_signature_clusters_seeded, Context.signature_clusters(seeds=...), `cluster --against`): the
device result equals an independent brute force byte for byte on the grid of drops and seed tables for every threshold and walk order, on
the planted cases in three placements and in the concatenation property against the unseeded device form; under every split of the seed
pass and of the walk's scan; the stage list; the refusals; the command on the device against --host and what its files are for."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from folddisco_amd import indexio
from tests import cluster_cases as cc
from tests import seeded_cluster_cases as scc
from tests.helpers import SER

pytestmark = pytest.mark.gpu

DT = indexio.SIGNATURE_NEIGHBOR_DTYPE
SEED_STAGES = ("sigcl_seed_upload", "sigcl_seed", "sigcl_seed_merge")


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", scc.NS)
def test_device_equals_brute_force(ctx, n):
    for nT in scc.NTS:
        S, T = scc.grid_tables(n, nT)
        void = T.copy()
        void["n"] = 0
        for thr in scc.THRESHOLDS:
            for name in scc.ORDERS:
                order = cc.order_of(S, name)
                w = scc.want(n, nT, thr, name)
                got = ctx.signature_clusters(S, order, thr64=thr, seeds=T)
                assert got.dtype == DT and got.shape == (n,)
                for f in DT.names:
                    assert np.array_equal(got[f], w[f]), (n, nT, thr, name, f)
                assert got.tobytes() == w.tobytes()
            plain = ctx.signature_clusters(S, order, thr64=thr)
            if nT == 0:
                assert got.tobytes() == plain.tobytes()
            assert ctx.signature_clusters(S, order, thr64=thr, seeds=void).tobytes() == plain.tobytes(), (n, nT, thr)      # flags included
            assert ctx.signature_clusters(S, None, thr64=thr, seeds=T).tobytes() == scc.want(n, nT, thr, "identity").tobytes()


@pytest.mark.parametrize("cell", scc.CONCAT_CELLS)
def test_concatenation_property(ctx, cell):
    n, nT = cell
    Bt, A = scc.grid_tables(n, nT)
    oA, oB, joined_order = scc.concat_orders(A, Bt)
    for thr in (32, 48):
        joined = ctx.signature_clusters(np.concatenate([A, Bt]), joined_order, thr64=thr)
        RA, w = scc.concat_expected(joined, nT, DT)
        assert 0 < len(RA) <= nT and (w["flags"] & scc.SEED).any()
        assert ctx.signature_clusters(Bt, oB, thr64=thr, seeds=A[RA]).tobytes() == w.tobytes(), (cell, thr)


def test_planted_cases(ctx):
    for name, S, T, order, thr, expect, w in scc.planted_want():
        got = ctx.signature_clusters(S, order, thr64=thr, seeds=T)
        assert scc.named(got, expect) == expect, name
        assert got.tobytes() == w.tobytes(), name


@pytest.mark.parametrize("cell", scc.SPLIT_CELLS)
def test_every_split_gives_the_same_bytes(ctx, cell, monkeypatch):
    S, T = scc.grid_tables(*cell)
    order, thr = cc.order_of(S, "random"), 48
    want = scc.want(*cell, thr, "random").tobytes()
    for var in ("FDGPU_SG_CL_SEED_SPLIT", "FDGPU_SG_CL_SPLIT"):
        monkeypatch.delenv(var, raising=False)
    assert ctx.signature_clusters(S, order, thr64=thr, seeds=T).tobytes() == want
    for seed_split in scc.SEED_SPLITS:
        for split in scc.WALK_SPLITS:
            monkeypatch.setenv("FDGPU_SG_CL_SEED_SPLIT", str(seed_split))      # both are read per call
            monkeypatch.setenv("FDGPU_SG_CL_SPLIT", str(split))
            assert ctx.signature_clusters(S, order, thr64=thr, seeds=T).tobytes() == want, (cell, seed_split, split)
    for var in ("FDGPU_SG_CL_SEED_SPLIT", "FDGPU_SG_CL_SPLIT"):
        monkeypatch.delenv(var, raising=False)
    assert ctx.signature_clusters(S, order, thr64=thr, seeds=T).tobytes() == want      # two runs give the same bytes


def test_stages_and_refusals(ctx, monkeypatch):
    import folddisco_amd as fd
    monkeypatch.delenv("FDGPU_SG_CL_SEED_SPLIT", raising=False)
    S, T = scc.grid_tables(513, 700)
    ctx.enable_timing(True)
    ok = ctx.signature_clusters(S, thr64=32, seeds=T)
    stages = [s for s, _, _ in ctx.last_timings()]
    first = stages.index("sigcl_resolve")
    assert all(stages.count(s) == 1 and stages.index(s) < first for s in SEED_STAGES), stages      # eleven tiles of seeds over three blocks: split
    assert [s for s in stages if s not in SEED_STAGES] == ["sigcl_upload", "sigcl_resolve", "sigcl_scan", "sigcl_resolve", "sigcl_scan", "sigcl_resolve", "sigcl_copy"]
    monkeypatch.setenv("FDGPU_SG_CL_SEED_SPLIT", "1")
    assert ctx.signature_clusters(S, thr64=32, seeds=T).tobytes() == ok.tobytes()
    one = [s for s, _, _ in ctx.last_timings()]
    assert "sigcl_seed_merge" not in one and one.count("sigcl_seed") == 1 and one.count("sigcl_seed_upload") == 1
    monkeypatch.delenv("FDGPU_SG_CL_SEED_SPLIT")
    ctx.signature_clusters(S, thr64=32, seeds=T[:0])                           # no seeds: the stages of the unseeded call
    assert not set(SEED_STAGES) & {s for s, _, _ in ctx.last_timings()}
    ctx.signature_clusters(S, thr64=32, seeds=T)
    good = np.arange(513, dtype=np.uint32)
    twice = good.copy()
    twice[7] = 8
    s, t = S.ctypes.data, T.ctypes.data
    for args in ((s, 513, None, t, 700, 0), (s, 513, None, t, 700, 65), (s, 1 << 32, None, t, 700, 32), (None, 3, None, t, 700, 32), (s, 513, None, None, 700, 32),
                 (s, 513, None, t, 0xffffffff - 512, 32), (s, 513, None, t, 1 << 32, 32), (s, 513, twice.ctypes.data, t, 700, 32)):
        out = C.c_void_p(1)
        assert ctx.L.fdgpu_signature_clusters_seeded(ctx.h, *args, C.byref(out)) == -1 and not out, args[1:]
        assert ctx.L.fdgpu_last_error(ctx.h).decode().startswith("signature clusters:")
    for kw in (dict(thr64=0), dict(thr64=65)):
        with pytest.raises(fd.FdgpuError, match="signature clusters:"):
            ctx.signature_clusters(S, seeds=T, **kw)
    with pytest.raises(ValueError, match="^signature clusters:"):
        ctx.signature_clusters(S, good[:5], seeds=T)
    with pytest.raises(ValueError, match="^seeds:"):
        ctx.signature_clusters(S, seeds=np.zeros(3, np.uint32))
    assert [s for s, _, _ in ctx.last_timings()] == stages                     # the refused calls recorded no stage: nothing was launched
    ctx.enable_timing(False)
    assert ctx.signature_clusters(S[:0], seeds=T).shape == (0,)
    assert ctx.signature_clusters(S, thr64=32, seeds=T).tobytes() == ok.tobytes()      # the context is usable afterwards


def _cli(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


def _rows(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def test_cli_cluster_against(tmp_path, capsys):
    """the serine peptidases split into a database of three and a drop of the two others plus copies of two database files under other
    names: the copies join their originals; after `update --remove` of the listed members the drop adds nothing the database has"""
    n_db = 3
    dirs = {"db": [(p, os.path.basename(p)) for p in SER[:n_db]],
            "drop": [(p, os.path.basename(p)) for p in SER[n_db:]] + [(p, "copy_" + os.path.basename(p)) for p in SER[:2]]}
    prefix = {}
    for name, files in dirs.items():
        d = str(tmp_path / name)
        os.makedirs(d)
        for src, dst in files:
            shutil.copy(src, os.path.join(d, dst))
        prefix[name] = str(tmp_path / f"ix_{name}")
        assert _cli(["index", "-p", d, "-i", prefix[name]]) == 0
    db, drop = prefix["db"], prefix["drop"]
    n_drop = len(dirs["drop"])
    f = {k: str(tmp_path / k) for k in ("dev.tsv", "host.tsv", "red.txt", "red_host.txt", "reps.txt", "reps_host.txt")}
    sim = "0.5"
    capsys.readouterr()
    common = ["cluster", "-i", drop, "--against", db, "--confirm", "--rep-by", "id", "--min-similarity", sim]
    assert _cli(common + ["-o", f["dev.tsv"], "--redundant", f["red.txt"], "--representatives", f["reps.txt"], "--window", "3", "--verify"]) == 0
    line = capsys.readouterr().out
    assert _cli(common + ["-o", f["host.tsv"], "--redundant", f["red_host.txt"], "--representatives", f["reps_host.txt"], "--host", "-t", "2"]) == 0
    assert capsys.readouterr().out == line
    for a, b in (("dev.tsv", "host.tsv"), ("red.txt", "red_host.txt"), ("reps.txt", "reps_host.txt")):
        assert open(f[a]).read() == open(f[b]).read(), a
    rows = _rows(f["dev.tsv"])
    assert all(len(c) == 12 for c in rows)
    assert [(c[10] != "against", int(c[0]), int(c[3])) for c in rows] == sorted((c[10] != "against", int(c[0]), int(c[3])) for c in rows)
    name = os.path.basename                                                    # a tid is the file's path
    copies = [c for c in rows if name(c[4]).startswith("copy_")]
    assert len(copies) == 2 and all(c[9] == "identical" and c[10] == "against" and c[11] == "1.0000" and name(c[4]) == "copy_" + name(c[1]) for c in copies)
    n_seed_members = sum(c[10] == "against" for c in rows)
    n_rep = sum(c[9] == "representative" for c in rows)
    assert line.startswith(f"[OK] {drop} x {db}: {n_drop} x {n_db} structures, {n_db} seeds, {n_rep} new clusters (") and line.endswith(", threshold 32/64\n")
    assert f"), {n_seed_members} members of seeds, {len(rows) - n_rep - n_seed_members} members of new representatives (" in line
    members = open(f["red.txt"]).read().splitlines()
    assert len(members) == len(rows) - n_rep >= 2 and open(f["reps.txt"]).read().splitlines() == [c[4] for c in sorted(rows, key=lambda c: int(c[3])) if c[9] == "representative"]
    # what the list is for: the drop without its members, joined to the database, has no pair of a kept drop structure and a seed
    kept, joined, pairs = str(tmp_path / "kept"), str(tmp_path / "joined"), str(tmp_path / "dups.tsv")
    assert _cli(["update", "-i", drop, "--remove", f["red.txt"], "-o", kept]) == 0
    assert _cli(["merge", "-i", db, kept, "-o", joined]) == 0
    assert _cli(["dups", "-i", joined, "-o", pairs, "--min-similarity", sim]) == 0
    assert not [c for c in _rows(pairs) if int(c[0]) < n_db <= int(c[3])]
    # --against-reps with the database's own --representatives: the clusters of [db; drop] walked in that order (the concatenation property)
    db_reps, whole, both, seeded = (str(tmp_path / k) for k in ("db_reps.txt", "whole", "both.tsv", "seeded.tsv"))
    assert _cli(["cluster", "-i", db, "-o", str(tmp_path / "db.tsv"), "--representatives", db_reps, "--rep-by", "id", "--min-similarity", sim]) == 0
    assert _cli(["merge", "-i", db, drop, "-o", whole]) == 0
    assert _cli(["cluster", "-i", whole, "-o", both, "--rep-by", "id", "--min-similarity", sim]) == 0
    assert _cli(["cluster", "-i", drop, "--against", db, "--against-reps", db_reps, "-o", seeded, "--rep-by", "id", "--min-similarity", sim]) == 0
    predicted = []
    for c in _rows(both):
        if int(c[3]) < n_db:
            continue
        inside = int(c[0]) >= n_db
        predicted.append([str(int(c[0]) - n_db) if inside else c[0], c[1], c[2], str(int(c[3]) - n_db)] + c[4:] + ["self" if inside else "against"])
    assert sorted(_rows(seeded)) == sorted(predicted) and predicted
    # refusals: status 1 or 2, nothing written
    names = sorted(os.listdir(tmp_path))
    bad = str(tmp_path / "bad_reps.txt")
    out = str(tmp_path / "never.tsv")
    assert _cli(["cluster", "-i", drop, "--against", drop, "-o", out]) == 2
    assert _cli(["cluster", "-i", drop, "--against", str(tmp_path / "nope"), "-o", out]) == 2
    assert _cli(["cluster", "-i", drop, "--against-reps", db_reps, "-o", out]) == 1
    assert _cli(["cluster", "-i", drop, "--against", db, "--against-reps", bad, "-o", out]) == 2
    assert sorted(os.listdir(tmp_path)) == names
    with open(bad, "w") as fh:
        fh.write("no_such_tid\n")
    assert _cli(["cluster", "-i", drop, "--against", db, "--against-reps", bad, "-o", out, "--representatives", str(tmp_path / "never.txt")]) == 1
    assert sorted(os.listdir(tmp_path)) == sorted(names + ["bad_reps.txt"])
    assert not [x for x in os.listdir(tmp_path) if "cluster-tmp" in x]
