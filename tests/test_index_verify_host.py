"""Index verification on the host (fdgpu_verify_host, indexio.verify_host / check_index_files, `verify --host`): the library's report equals the
plain Python checker of tests/index_verify_cases.py, field by field, on clean indices, on directed damage of every class and on seeded
random damage.  No GPU.

Seeded damage, share of the damaged cases that the yardstick reports bad (seed 1; the floors 0.9 / 0.4 are asserted on the value replacements and on
all cases): serine index 1977 of the 2,000 value replacements (0.9885), 200 of 200 offsets, 111 of 200 hashes (0.953 of all 2,400);
synthetic 600-structure index 1180 of 2,000 value replacements (0.59), 190 of 200 offsets, 141 of 200 hashes (0.630 of all)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from tests import helpers
from tests import index_verify_cases as ivc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(c, threads=3):
    from folddisco_amd import indexio
    return ivc.report_dict(indexio.verify_host(c["value"], c["hashes"], c["offsets"], c["n_structures"], c["first_id"], threads=threads))


def _check_expect(c, rep):
    if c["expect"] is None:
        assert rep["ok"] and rep["n_bad"] == 0 and rep["n_lists"] == len(c["hashes"]), (c["name"], rep)
        assert rep["n_postings"] == int((c["value"] < 0x80).sum()), c["name"]
        return
    cls, slot = c["expect"]
    cls = (cls,) if isinstance(cls, int) else cls
    assert not rep["ok"] and rep["n_bad"] == 1 and rep["first_slot"] == slot, (c["name"], rep)
    assert rep["first_classes"] == tuple(ivc.CLASSES[x - 1] for x in cls), (c["name"], rep)      # exactly that class: none of 6-8 behind 4 / 5
    assert rep["counts"] == {n: int(k + 1 in cls) for k, n in enumerate(ivc.CLASSES)}, (c["name"], rep)


@pytest.fixture(scope="module")
def serine():
    structs = [oracle.read_pdb(p) for p in helpers.SER]
    ix, _, _ = oracle.build_index(structs)
    return ix.values().copy(), ix.hashes().copy(), ix.offsets().copy(), len(structs)


@pytest.fixture(scope="module")
def synth600():
    structs = helpers.packed_to_oracle_structs(helpers.synthetic_packed(600, 7))
    ix, _, _ = oracle.build_index(structs)
    return ix.values().copy(), ix.hashes().copy(), ix.offsets().copy(), len(structs)


def test_clean_hand_encoded_indices():
    names = []
    for c in ivc.clean_cases():
        want = ivc.py_verify(c["value"], c["hashes"], c["offsets"], c["n_structures"], c["first_id"])
        _check_expect(c, want)
        for threads in (1, 4):
            assert _host(c, threads) == want, c["name"]
        names.append(c["name"])
    assert names == ["hand", "hand_shard", "empty", "one_list"]
    hand = next(ivc.clean_cases())
    lens = np.diff(hand["offsets"].astype(np.int64))
    assert lens.max() > 65536 and lens.min() == 1 and {len(ivc.varint(v)) for v in (5, 194, 20000, 3000000, 0x20000000)} == {1, 2, 3, 4, 5}


def test_clean_serine_index(serine):
    v, h, o, S = serine
    want = ivc.py_verify(v, h, o, S)
    assert want["ok"] and want["n_lists"] == len(h) and want["n_postings"] == int((v < 0x80).sum()) and want["max_id"] == S - 1
    from folddisco_amd import indexio
    assert ivc.report_dict(indexio.verify_host(v, h, o, S, threads=4)) == want
    # the same lists as a shard that was loaded without its first id: the ids run past n_structures
    assert not indexio.verify_host(v, h, o, S - 1).ok


def test_directed_damage_every_class():
    seen = set()
    n = 0
    for c in ivc.directed_cases():
        want = ivc.py_verify(c["value"], c["hashes"], c["offsets"], c["n_structures"], c["first_id"])
        _check_expect(c, want)
        assert _host(c) == want, c["name"]
        if c["expect"]:
            seen |= set((c["expect"][0],) if isinstance(c["expect"][0], int) else c["expect"][0])
        n += 1
    assert seen == set(range(1, 9)) and n > 300


def _seeded(v, h, o, S, n_value, n_table, base, threads):
    from folddisco_amd import indexio
    v, h, o = v.copy(), h.copy(), o.copy()
    bad = {"value": 0, "offsets": 0, "hashes": 0}
    tot = {"value": 0, "offsets": 0, "hashes": 0}
    for kind, pos, lists in ivc.seeded_cases(v, h, o, 1, n_value, n_table):
        want = ivc.py_verify(v, h, o, S, only=lists, base=base)
        got = ivc.report_dict(indexio.verify_host(v, h, o, S, threads=threads))
        assert got == want, (kind, pos)
        tot[kind] += 1
        bad[kind] += not want["ok"]
    return bad, tot


def test_seeded_damage_serine(serine):
    v, h, o, S = serine
    base = ivc.np_list_arrays(v, o)
    full = ivc.py_verify(v, h, o, S)
    assert int(base[0].sum()) == full["n_postings"] and int(base[1].max()) == full["max_id"]      # the vectorised start state is the yardstick's
    bad, tot = _seeded(v, h, o, S, 2000, 200, base, 2)
    print("serine: reported bad", bad, "of", tot)
    assert tot == {"value": 2000, "offsets": 200, "hashes": 200}
    assert sum(bad.values()) / sum(tot.values()) >= 0.9 and bad["value"] / tot["value"] >= 0.9


def test_seeded_damage_synthetic(synth600):
    v, h, o, S = synth600
    base = ivc.np_list_arrays(v, o)
    from folddisco_amd import indexio
    clean = indexio.verify_host(v, h, o, S, threads=8)
    assert clean.ok and clean.n_postings == int(base[0].sum()) == int((v < 0x80).sum()) and clean.max_id == int(base[1].max()) == S - 1
    assert clean.max_list_bytes == int(np.diff(o.astype(np.int64)).max())
    bad, tot = _seeded(v, h, o, S, 2000, 200, base, 8)
    print("synthetic: reported bad", bad, "of", tot)
    assert sum(bad.values()) / sum(tot.values()) >= 0.4 and bad["value"] / tot["value"] >= 0.4


# ---- files and the command -----------------------------------------------------------------------------------------------------------
def write_prefix(d, v, h, o, S, name="ix"):
    from folddisco_amd import indexio
    p = os.path.join(str(d), name)
    indexio.write_index_files(p, v, h, o)
    indexio.save_lookup_py(p + ".lookup", [f"s{k}.pdb" for k in range(S)], np.full(S, 100), np.full(S, 50.0, np.float32))
    indexio.save_type(p + ".type", S)
    return p


def test_check_index_files(tmp_path, serine):
    from folddisco_amd import indexio
    v, h, o, S = serine
    p = write_prefix(tmp_path, v, h, o, S)
    assert indexio.check_index_files(p) == []
    raw = open(p + ".offset", "rb").read()

    def one_complaint(about):
        bad = indexio.check_index_files(p)
        assert len(bad) == 1 and about in bad[0], bad

    open(p + ".offset", "wb").write(raw[:-8])
    one_complaint(".offset")
    open(p + ".offset", "wb").write(raw + b"\0" * 4)
    one_complaint(".offset")
    open(p + ".offset", "wb").write(raw)
    v[:-1].tofile(p)
    one_complaint("last offset")
    v.tofile(p)
    rows = open(p + ".lookup").readlines()
    open(p + ".lookup", "w").writelines(rows[:2] + rows[3:])
    bad = indexio.check_index_files(p)
    assert len(bad) == 2 and "row 3" in bad[0] and "chunk_size" in bad[1], bad
    open(p + ".lookup", "w").writelines(rows)
    indexio.save_type(p + ".type", S + 1)
    one_complaint("chunk_size")
    indexio.save_type(p + ".type", S)
    assert indexio.check_index_files(p) == []
    os.remove(p + ".type")
    one_complaint("not found")


# runs the command with Context replaced by something that fails: `verify --host` must not open a device
_NO_CONTEXT = ("import sys, folddisco_amd as fd, folddisco_amd.api as api\n"
               "def boom(*a, **k): raise SystemExit('a context was created')\n"
               "fd.Context = api.Context = boom\n"
               "from folddisco_amd.__main__ import main\n"
               "main(sys.argv[1:])\n")


def _verify_host_cli(prefix, *more):
    return subprocess.run([sys.executable, "-c", _NO_CONTEXT, "verify", "--host", "-i", prefix, *more], cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_verify_command_on_the_host(tmp_path, serine):
    v, h, o, S = serine
    p = write_prefix(tmp_path, v, h, o, S)
    r = _verify_host_cli(p, "-t", "2", "-v")
    assert r.returncode == 0, r.stderr
    line = r.stdout.strip().splitlines()
    assert len(line) == 1 and line[0].startswith("[OK]") and f"{len(h)} lists" in line[0] and f"{int((v < 0x80).sum())} postings" in line[0] \
        and f"max id {S - 1}" in line[0]
    # one byte of the value file damaged: a continuation bit on the last byte of list 1000
    d = v.copy()
    d[int(o[1001]) - 1] |= 0x80
    p2 = write_prefix(tmp_path, d, h, o, S, "damaged")
    r = _verify_host_cli(p2)
    assert r.returncode == 1, r.stderr
    line = r.stdout.strip().splitlines()
    assert len(line) == 1 and line[0].startswith("[FAIL]") and "slot 1000" in line[0] and f"hash {int(h[1000])}" in line[0] and "LIST_END" in line[0] \
        and "LIST_END 1" in line[0]
    # files that contradict each other: status 1 before any decoding; a missing file: status 2
    v[:-1].tofile(p)
    r = _verify_host_cli(p)
    assert r.returncode == 1 and r.stdout.startswith("[FAIL]") and "last offset" in r.stdout
    os.remove(p + ".offset")
    assert _verify_host_cli(p).returncode == 2
