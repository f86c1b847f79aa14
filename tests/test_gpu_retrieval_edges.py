"""fdgpu_retrieve_batch and the pair scan on the hand-made query maps of retrieval_cases.py, at the limits and form switches of the retrieval's dispatch,
against the oracle (test_retrieval_cases_host.py checks on the CPU that every case sits where it claims to sit).

Per case (the limit candidate and the ordinary one beside it in one call): every record against oracle.retrieve — candidate slot, from-hash and
processed residues and the `same` flag exactly, records ordered by slot and then like the reference orders components, idf bit for bit (every idf is
a multiple of 2^-8), rmsd and rmsd_from_hash within 1e-4 (the project's RMSD bound).  Then the same call under each of FORMS: the four output tables
byte for byte equal to the default form's.  FDGPU_PACK_MIN applies only where the host path receives the candidate pairs packed (it is read by the scan
that fdgpu_retrieve_batch's host path starts, not by fdgpu_match_pairs), so it is run together with FDGPU_HOST_GLUE=1; FDGPU_DEVICE_VOTES=0 changes
something only in a two-pass call, so it is also run together with FDGPU_TWO_PASS=1.

Which way a call went is read from the stage names (ctx.last_timings: "retrieve_slots" present = the device glue ran; an abandoned device attempt
restarts the list at "match_pairs") and from fdgpu_debug_last_retrieve_path, since stage names alone cannot tell a declined device attempt from a call
that never started one (overflow cases: 65 nodes, 1,025 found triples, 65 voted query residues, the rescue lists' caps).  Neither tells whether a slot listed by k_rs_setup was then processed by k_rs_slots, nor whether the candidate pairs were read
from LDS or from global memory: those switches (RS_S_EDGE, RS_CAND_LDS, RS_S_FILT, the LDS copies of the hash set) are covered by results only — a case
on either side, equal to the oracle and to FDGPU_RS_SPLIT=0.

Pair scan alone: match.match_pairs on the window, sizes and long cases == the oracle's found and cand arrays exactly, in (i, j, emission) order.
Batching: an in-limit, an overflowing and an empty-result query in one call and each alone give the same tables per query.
Measured: the module's 13 tests take 6 s on an MI355X, the slowest (the rescue class: 17 cases x 9 forms) 1.9 s."""
import ctypes as C

import numpy as np
import pytest

from tests import retrieval_cases as rc

pytestmark = pytest.mark.gpu

TRIED, DONE, LIMIT, CAPACITY, TWO_PASS, SPLIT = 1, 2, 4, 8, 16, 32
FORMS = ({"FDGPU_HOST_GLUE": "1"}, {"FDGPU_RS_SPLIT": "0"}, {"FDGPU_MP_ITEMS": "0"}, {"FDGPU_DEVICE_VOTES": "0"}, {"FDGPU_FOUND_SORT": "device"}, {"FDGPU_TWO_PASS": "1"},
         {"FDGPU_TWO_PASS": "1", "FDGPU_DEVICE_VOTES": "0"}, {"FDGPU_HOST_GLUE": "1", "FDGPU_PACK_MIN": "1"})
FORM_KEYS = sorted({k for f in FORMS for k in f})
TABLES = ("matches", "match_off", "residues", "res_off")


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


def last_path(ctx):
    f = C.c_uint32(0)
    ctx.check(ctx.L.fdgpu_debug_last_retrieve_path(ctx.h, C.byref(f)))
    return f.value


def upload(ctx, structs):
    import folddisco_amd as fd
    return ctx.upload(fd.PackedStructures.concat([s.item for s in structs]))


def run(ctx, monkeypatch, env, db, cands, qms, qb, q_structs, cutoff, node_count):
    from folddisco_amd import query as fq
    for k in FORM_KEYS:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)
    ctx.enable_timing(True)
    out = fq.retrieve_batch(ctx, db, None, cands, qms, qb, q_structs, ca_distance_cutoff=cutoff, node_count=node_count, as_arrays=True)
    ctx.synchronize()
    names = [n for n, _, _ in ctx.last_timings()]
    ctx.enable_timing(False)
    path = last_path(ctx)
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)
    return out, names, path


def check_against_oracle(c, tables):
    marr, moff, rarr, roff = tables
    nq = len(c.arrays["indices"])
    want = [(k, fh, pr) for k, R in enumerate(rc.oracle_results(c)) for fh, pr in zip(R["from_hash"], R["processed"])]
    assert moff.tolist() == [0, len(want)] and roff.tolist() == [0, 2 * nq * len(want)], (c, moff, len(want))
    res = rarr.reshape(len(want), 2, nq) if want else rarr.reshape(0, 2, nq)
    for x, (k, fh, pr) in enumerate(want):
        m = marr[x]
        f = [-1 if r is None else r[2] for r in fh["residues"]]
        p = [-1 if r is None else r[2] for r in pr["residues"]]
        assert int(m["cand"]) == k, (c, x)
        assert res[x, 0].tolist() == f and res[x, 1].tolist() == p, (c, x, res[x].tolist(), f, p)
        assert bool(m["same"]) == (f == p), (c, x)
        assert np.float32(m["idf"]).view(np.uint32) == np.float32(fh["idf"]).view(np.uint32), (c, x, float(m["idf"]), fh["idf"])
        assert abs(float(m["rmsd"]) - pr["rmsd"]) <= 1e-4 and abs(float(m["rmsd_from_hash"]) - fh["rmsd"]) <= 1e-4, (c, x)


def expected_path(c, env):
    """(device glue started, finished, declined for a limit) restated from the dispatch: <= 64 query residues, one scan, FDGPU_HOST_GLUE unset"""
    two_pass = env.get("FDGPU_TWO_PASS") == "1" or len(c.arrays["aad_dist"]) > rc.TWO_PASS_AAD
    tried = env.get("FDGPU_HOST_GLUE") != "1" and not two_pass and len(c.arrays["indices"]) <= rc.WAVE
    over = c.path == "overflow" and not (c.split_only and env.get("FDGPU_RS_SPLIT") == "0")          # (a limit of the split form alone: k_rs_slots finishes)
    return tried, tried and (c.path == "device" or c.path == "overflow" and not over), tried and over, two_pass


def run_case(ctx, monkeypatch, c):
    db, qb = upload(ctx, c.targets), upload(ctx, [c.query])
    qm = rc.library_map(c.arrays)
    args = (db, [np.arange(len(c.targets), dtype=np.uint32)], [qm], qb, [0], c.ca_distance_cutoff, c.node_count)
    base, names, path = run(ctx, monkeypatch, {}, *args)
    check_against_oracle(c, base)
    for env in ({},) + FORMS:
        if env:
            alt, names, path = run(ctx, monkeypatch, env, *args)
            for a, b, what in zip(base, alt, TABLES):
                assert a.tobytes() == b.tobytes(), (c, env, what)
        tried, done, limit, two_pass = expected_path(c, env)
        assert bool(path & TRIED) == tried and bool(path & DONE) == done and bool(path & LIMIT) == limit and not path & CAPACITY, (c, env, hex(path))
        assert bool(path & TWO_PASS) == two_pass and bool(path & SPLIT) == (tried and env.get("FDGPU_RS_SPLIT") != "0"), (c, env, hex(path))
        assert ("retrieve_slots" in names) == done, (c, env, names)          # (an abandoned device attempt leaves no stage behind: the list restarts)
        if limit:
            assert names == ["match_pairs"], (c, env, names)


@pytest.mark.parametrize("cls", rc.CLASSES)
def test_retrieval_equals_oracle_in_every_form(ctx, cls, monkeypatch):
    cases = rc.cases(cls)
    assert cases
    for c in cases:
        run_case(ctx, monkeypatch, c)


@pytest.mark.parametrize("cls", ("window", "sizes", "long"))
def test_pair_scan_equals_oracle(ctx, cls, monkeypatch):
    from folddisco_amd import match
    for c in rc.cases(cls):
        db = upload(ctx, c.targets)
        for env in ({}, {"FDGPU_MP_ITEMS": "0"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            found, cands = match.match_pairs(ctx, db, None, np.arange(len(c.targets), dtype=np.uint32), rc.match_query(c.arrays), ca_distance_cutoff=c.ca_distance_cutoff)
            for k in env:
                monkeypatch.delenv(k)
            for k, R in enumerate(rc.oracle_results(c)):
                f, cd = found[found[:, 0] == k][:, 1:], cands[cands[:, 0] == k][:, 1:]
                assert np.array_equal(f.astype(np.uint64), R["found"]), (c, env, k)
                assert np.array_equal(cd.astype(np.uint64), R["cand"]), (c, env, k)


def test_batch_of_in_limit_overflow_and_empty_equals_single_calls(ctx, monkeypatch):
    """three queries over two query structures in one call: per query the tables of the call that holds it alone (the batch goes through the host path
    as a whole, because one of its slots overflows; the in-limit query alone takes the device glue)"""
    pick = {(c.cls, c.name): c for cls in ("comps", "nodes") for c in rc.cases(cls)}
    cs = [pick[("comps", "two_scc_one_way")], pick[("nodes", "chain65")], pick[("comps", "no_hash_found")]]
    assert [c.path for c in cs] == ["device", "overflow", "device"] and all(c.node_count == 2 and c.ca_distance_cutoff == 1.0 for c in cs)
    structs, q_structs, cands = [], [], []
    for c in cs:
        for s in [c.query] + c.targets:
            if s not in structs:
                structs.append(s)
        q_structs.append(structs.index(c.query))
        cands.append(np.array([structs.index(t) for t in c.targets], np.uint32))
    db = upload(ctx, structs)
    qms = [rc.library_map(c.arrays) for c in cs]
    (marr, moff, rarr, roff), names, path = run(ctx, monkeypatch, {}, db, cands, qms, db, q_structs, 1.0, 2)
    assert path & TRIED and path & LIMIT and not path & DONE and names == ["match_pairs"]
    assert moff[3] - moff[2] == 0 and moff[1] - moff[0] == 3 + len(rc.oracle_results(cs[0])[1]["from_hash"])
    for t, c in enumerate(cs):
        one, _, p1 = run(ctx, monkeypatch, {}, db, [cands[t]], [qms[t]], db, [q_structs[t]], 1.0, 2)
        assert bool(p1 & DONE) == (c.path == "device")
        check_against_oracle(c, one)
        assert marr[int(moff[t]):int(moff[t + 1])].tobytes() == one[0].tobytes() and rarr[int(roff[t]):int(roff[t + 1])].tobytes() == one[2].tobytes(), c


def test_path_flags_before_any_retrieval():
    import folddisco_amd as fd
    c = fd.Context(0)
    try:
        assert last_path(c) == 0
        assert c.L.fdgpu_debug_last_retrieve_path(c.h, None) != 0
    finally:
        c.close()
