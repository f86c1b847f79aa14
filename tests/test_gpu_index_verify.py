"""Index verification on the device (fdgpu_index_verify, FolddiscoIndex.verify, `verify`, `query --verify`, `update --verify`): the device report
equals the host checker's field by field over every clean, directed and seeded case of tests/index_verify_cases.py, the indices the library
makes verify clean, and the commands stop at a damaged index before anything else sees it.

A damaged index takes exactly one path on the GPU here: load -> verify -> destroy."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import index_verify_cases as ivc
from tests.helpers import SER

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


def _device(ctx, v, h, o, S, first_id=0):
    import folddisco_amd as fd
    ix = fd.FolddiscoIndex.load(ctx, h, o, v, S, first_id=first_id)
    rep = ix.verify()
    del ix
    return ivc.report_dict(rep)


def _host(v, h, o, S, first_id=0, threads=8):
    from folddisco_amd import indexio
    return ivc.report_dict(indexio.verify_host(v, h, o, S, first_id, threads=threads))


def test_clean_and_directed_cases_equal_the_host(ctx):
    n = 0
    for gen in (ivc.clean_cases, ivc.directed_cases):
        for c in gen():
            args = (c["value"], c["hashes"], c["offsets"], c["n_structures"], c["first_id"])
            want = _host(*args)
            assert want["ok"] == (c["expect"] is None), c["name"]
            assert _device(ctx, *args) == want, c["name"]
            n += 1
    assert n > 300


@pytest.mark.parametrize("kind", ["serine", "synth600"])
def test_seeded_damage_equals_the_host(ctx, kind):
    v, h, o, S = ivc.oracle_index(kind)
    clean = _host(v, h, o, S)
    assert clean["ok"] and _device(ctx, v, h, o, S) == clean
    bad = n = 0
    for what, pos, _ in ivc.seeded_cases(v, h, o, 1, 2000, 200):
        want = _host(v, h, o, S)
        assert _device(ctx, v, h, o, S) == want, (what, pos)
        bad += not want["ok"]
        n += 1
    assert n == 2400 and bad / n >= (0.9 if kind == "serine" else 0.4)


def _clean_with_totals(ix):
    rep = ix.verify()
    assert rep.ok and rep.n_bad == 0 and rep.list_stage, str(rep)
    assert rep.n_lists == ix.num_hashes and rep.n_postings == ix.num_postings
    assert rep.max_id < ix.first_id + ix.n_structures
    return rep


def test_indices_the_library_makes_verify_clean(ctx):
    import folddisco_amd as fd
    from folddisco_amd import synth
    ps = synth.to_packed(synth.generate(4400, seed=41))
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(ps))
    rep = _clean_with_totals(ix)
    v, h, o = ix.export()
    assert rep.max_id == ps.n_struct - 1 and rep.max_list_bytes == int(np.diff(o.astype(np.int64)).max())
    assert ivc.report_dict(rep) == _host(v, h, o, ps.n_struct)
    keep = np.random.Generator(np.random.PCG64(3)).random(ps.n_struct) >= 0.05
    pruned = ix.remove(keep)
    _clean_with_totals(pruned)
    add = synth.to_packed(synth.generate(60, seed=42))
    _clean_with_totals(pruned.append(ctx, ctx.upload(add)))
    # three parts merged, a slice of the merge
    off = ps.res_off.astype(np.int64)
    parts, cuts = [], [0, 1500, 2900, ps.n_struct]
    for a, b in zip(cuts, cuts[1:]):
        items = [dict(n_xyz=ps.n_xyz[off[s]:off[s + 1]], ca_xyz=ps.ca_xyz[off[s]:off[s + 1]], cb_xyz=ps.cb_xyz[off[s]:off[s + 1]], aa=ps.aa[off[s]:off[s + 1]])
                 for s in range(a, b)]
        parts.append(fd.FolddiscoIndex.build(ctx, ctx.upload(fd.PackedStructures.concat(items)), first_id=a))
    for p in parts:
        _clean_with_totals(p)
    merged = fd.FolddiscoIndexSet(parts).merge()
    assert ivc.report_dict(_clean_with_totals(merged)) == ivc.report_dict(rep)
    _clean_with_totals(merged.slice(int(h[len(h) // 3]), int(h[2 * len(h) // 3])))
    # a shard that went through the files: with its first id it is clean, without it its ids run past its structures
    sv, sh, so = parts[1].export()
    n1 = cuts[2] - cuts[1]
    shard = fd.FolddiscoIndex.load(ctx, sh, so, sv, n1, first_id=cuts[1])
    _clean_with_totals(shard)
    lost = fd.FolddiscoIndex.load(ctx, sh, so, sv, n1).verify()
    assert not lost.ok and lost.counts["ID_RANGE"] == lost.n_bad > 0 and set(lost.counts.values()) == {0, lost.n_bad}
    assert ivc.report_dict(lost) == _host(sv, sh, so, n1)


def test_verify_abi(ctx):
    import ctypes as C
    from folddisco_amd import _lib
    r = _lib.VerifyReportC()
    assert ctx.L.fdgpu_index_verify(ctx.h, None, C.byref(r)) == -1


# ---- the commands: one subprocess per case, each under its own time limit
def _cli(args, cwd, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "folddisco_amd", *args], cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)


def _files(prefix):
    return [open(prefix + ext, "rb").read() for ext in ("", ".offset", ".lookup", ".type")]


@pytest.fixture(scope="module")
def prefixes(tmp_path_factory):
    """a good index over four serine peptidases and a copy whose value file has one continuation bit too many"""
    from folddisco_amd import indexio
    d = tmp_path_factory.mktemp("verify_cli")
    (d / "db").mkdir()
    for p in SER[:4]:
        shutil.copy(p, d / "db" / os.path.basename(p))
    (d / "add").mkdir()
    shutil.copy(SER[4], d / "add" / os.path.basename(SER[4]))
    r = _cli(["index", "-p", "db", "-i", "good", "--id", "basename_without_ext"], d)
    assert r.returncode == 0, r.stderr
    for ext in ("", ".offset", ".lookup", ".type"):
        shutil.copy(str(d / "good") + ext, str(d / "bad") + ext)
    v, h, o = indexio.read_index_files(str(d / "bad"))
    k = len(h) // 2
    v[int(o[k + 1]) - 1] |= 0x80
    v.tofile(str(d / "bad"))
    return d, k, int(h[k])


def test_cli_verify_on_the_device(prefixes):
    d, k, hk = prefixes
    r = _cli(["verify", "-i", "good", "-v"], d)
    assert r.returncode == 0 and r.stdout.startswith("[OK]") and len(r.stdout.strip().splitlines()) == 1 and "device" in r.stderr, r.stderr
    host = _cli(["verify", "-i", "good", "--host"], d)
    assert host.returncode == 0 and host.stdout == r.stdout
    r = _cli(["verify", "-i", "bad"], d)
    assert r.returncode == 1 and r.stdout.startswith("[FAIL]") and f"slot {k} " in r.stdout and f"hash {hk}" in r.stdout and "LIST_END" in r.stdout, r.stderr
    assert _cli(["verify", "-i", "bad", "--host"], d).stdout == r.stdout
    assert _cli(["verify", "-i", "nosuch"], d).returncode == 2


def test_cli_query_verify_stops_at_a_damaged_index(prefixes):
    d, k, hk = prefixes
    q = ["query", "-p", os.path.join(GOLDEN, "query", "4CHA.pdb"), "-q", "B57,B102,C195", "--skip-match"]
    good = _cli(q + ["-i", "good", "--verify", "-o", "good.out"], d)
    plain = _cli(q + ["-i", "good", "-o", "plain.out"], d)
    assert good.returncode == 0 and plain.returncode == 0, good.stderr + plain.stderr
    assert open(d / "good.out").read() == open(d / "plain.out").read() != ""
    before = _files(str(d / "bad"))
    r = _cli(q + ["-i", "bad", "--verify", "-o", "bad.out"], d)
    assert r.returncode == 1 and r.stdout.startswith("[FAIL]") and f"slot {k} " in r.stdout and len(r.stdout.strip().splitlines()) == 1, r.stderr
    assert not os.path.exists(d / "bad.out") and _files(str(d / "bad")) == before


def test_cli_update_verify_stops_at_a_damaged_index(prefixes):
    d, k, hk = prefixes
    before = _files(str(d / "bad"))
    r = _cli(["update", "-i", "bad", "-p", "add", "--id", "basename_without_ext", "--verify"], d)
    assert r.returncode == 1 and r.stdout.startswith("[FAIL]") and f"slot {k} " in r.stdout, r.stderr
    assert _files(str(d / "bad")) == before and not [f for f in os.listdir(d) if "update-tmp" in f]
    # a sound index: the same files with and without the flag
    for name in ("up1", "up2"):
        for ext in ("", ".offset", ".lookup", ".type"):
            shutil.copy(str(d / "good") + ext, str(d / name) + ext)
    r1 = _cli(["update", "-i", "up1", "-p", "add", "--id", "basename_without_ext", "--verify"], d)
    r2 = _cli(["update", "-i", "up2", "-p", "add", "--id", "basename_without_ext"], d)
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
    assert _files(str(d / "up1")) == _files(str(d / "up2")) != _files(str(d / "good"))
    assert _cli(["verify", "-i", "up1"], d).returncode == 0
