"""The quantiser edge sets (tests/quantiser_edges.py) through the C ABI on the GPU: every product — raw S1 lists, index bytes under the four build
forms, the speculation's fallback counter, query maps, count records, retrieval — equals the oracle's, byte for byte, on inputs that sit one ulp
to either side of a quantiser threshold or of the accept test, and with cutoffs other than 20 A.  There is no tolerance on anything a hash decides;
RMSD / idf keep the tolerances of tests/test_gpu_e2e.py.

Standing check of the proof obligations of fd_pair_both_spec (fd_geom.h): an accepted speculative decision next to a threshold is compared with
the exact arithmetic here (the ladders), not only the fallback."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from tests import quantiser_edges as qe
from tests.helpers import Q4CHA, SER, oracle_structs_to_packed

pytestmark = pytest.mark.gpu
BUILD_FORMS = ({}, {"FDGPU_DTAB": "0"}, {"FDGPU_EXACT": "1"}, {"FDGPU_MSD": "0"})


@pytest.fixture(scope="module")
def gpu():
    """one context for the module; the process gives itself a time limit (a hung kernel ends the run instead of holding the device)"""
    import folddisco_amd as fd
    faulthandler.dump_traceback_later(1500, exit=True)
    ctx = fd.Context(0)
    yield ctx, qe.all_sets()
    ctx.close()
    faulthandler.cancel_dump_traceback_later()


def _set_env(monkeypatch, form):
    for k in ("FDGPU_DTAB", "FDGPU_EXACT", "FDGPU_MSD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in form.items():
        monkeypatch.setenv(k, v)


def _layouts(X, aa, cell, packed=True):
    out = [("per pair", qe.layout_per_pair(X, aa))]
    if packed and aa.shape[1] == 2:
        out.append(("packed", qe.layout_packed(X, aa, cell)))
    return out


def _assert_s1(ctx, d, cfg, name):
    import folddisco_amd as fd
    batch = ctx.upload(qe.to_packed(d))
    h, off = fd.get_geometric_hash_as_u32(ctx, batch, nbin_dist=cfg.nd, nbin_angle=cfg.na, dist_cutoff=cfg.cutoff, sort_dedup=False, hash_type=cfg.hash_type)
    wh, woff = qe.oracle_lists(d, cfg)
    assert np.array_equal(off, woff), (name, int(np.argmax(np.diff(off.astype(np.int64)) != np.diff(woff.astype(np.int64)))))
    bad = np.nonzero(h != wh)[0]
    assert len(bad) == 0, (name, len(bad), int(np.searchsorted(woff, bad[0], side="right") - 1), hex(int(h[bad[0]])), hex(int(wh[bad[0]])))
    return len(h)


def test_raw_s1_lists_equal_oracle_on_every_edge_set(gpu):
    ctx, S = gpu
    n = 0
    for key in ("default", "origin"):
        for lname, d in _layouts(*S[key].sides(), packed=key == "default"):
            n += _assert_s1(ctx, d, qe.DEFAULT, f"{key} {lname}")
    X, aa, cell, _ = S["ladder"]
    for lname, d in _layouts(X, aa, cell):
        n += _assert_s1(ctx, d, qe.DEFAULT, f"ladder {lname}")
    for es in list(S["cutoff"].values()) + [v for v, _ in S["config"].values()]:
        for lname, d in _layouts(*es.sides()):
            n += _assert_s1(ctx, d, es.cfg, f"{es.cfg.name} {lname}")
    assert n > 300000


def _export_forms(ctx, monkeypatch, batch, **kw):
    import folddisco_amd as fd
    out = []
    for form in BUILD_FORMS:
        _set_env(monkeypatch, form)
        ctx.spec_fallbacks()
        out.append(fd.FolddiscoIndex.build(ctx, batch, **kw).export())
        n = ctx.spec_fallbacks()
        assert form.get("FDGPU_EXACT") != "1" or n == 0
    _set_env(monkeypatch, {})
    return out


def _assert_index(got, oix, name):
    v, h, o = got
    assert np.array_equal(h, oix.hashes()), name
    assert np.array_equal(o, oix.offsets()), name
    assert np.array_equal(v, oix.values()), name


@pytest.mark.parametrize("layout", ["per pair", "packed"])
def test_index_build_forms_equal_oracle_on_default_edges(gpu, monkeypatch, layout):
    """default form (speculation + distance table), FDGPU_DTAB=0, FDGPU_EXACT=1, FDGPU_MSD=0: each equals oracle.build_index byte for byte, so
    all four equal each other"""
    ctx, S = gpu
    X, aa, cell = S["default"].sides()
    Xl, aal, celll, _ = S["ladder"]
    d = dict(_layouts(np.concatenate([X, Xl[::4]]), np.concatenate([aa, aal[::4]]), np.concatenate([cell, celll[::4]])))[layout]
    oix, _, _ = oracle.build_index(qe.to_oracle_structs(d))
    forms = _export_forms(ctx, monkeypatch, ctx.upload(qe.to_packed(d)))
    for form, got in zip(BUILD_FORMS, forms):
        _assert_index(got, oix, (layout, form))
    for got in forms[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(forms[0], got))


@pytest.mark.parametrize("name", ["pdbtr_8_4", "pdbtr_12_4", "multiple_bins"])
def test_index_build_forms_equal_oracle_without_the_distance_table(gpu, monkeypatch, name):
    """PDBTrRosetta with 4 angle bins and 8 / 12 distance bins (speculative torsions, sqrt + quantiser distances), and a --multiple-bins list
    that mixes the table configuration with a non-table one, on their own edge sets plus the default edges"""
    ctx, S = gpu
    X, aa, cell = S["default"].sides()
    if name == "multiple_bins":
        bins, kw, okw = [(16, 4), (8, 3)], dict(multiple_bins=[(16, 4), (8, 3)]), {}
    else:
        es = S["config"][name][0]
        X2, aa2, cell2 = es.sides()
        X, aa, cell = np.concatenate([X2, X]), np.concatenate([aa2, aa]), np.concatenate([cell2, cell])
        bins, kw, okw = None, dict(nbin_dist=es.cfg.nd, nbin_angle=es.cfg.na), dict(nbin_dist=es.cfg.nd, nbin_angle=es.cfg.na)
    for lname, d in _layouts(X, aa, cell):
        structs = qe.to_oracle_structs(d)
        if bins:
            with oracle.multiple_bins(bins):
                oix, _, _ = oracle.build_index(structs)
        else:
            oix, _, _ = oracle.build_index(structs, **okw)
        forms = _export_forms(ctx, monkeypatch, ctx.upload(qe.to_packed(d)), **kw)
        for form, got in zip(BUILD_FORMS, forms):
            _assert_index(got, oix, (name, lname, form))
        for got in forms[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(forms[0], got))


def test_fallback_counter_on_edges_and_ladders(gpu, monkeypatch):
    """Every torsion edge drawn at the origin must fall back, on both of its sides.  The speculative path may accept a decision only when
    |g| = ||y| - t|x|| exceeds M = E_y + t E_x with E_y, E_x >= FD_SPEC_E1 = 7.6e-6 (fd_geom.h).  Across a torsion edge the reference's decision
    flips, so g changes sign between the two sides, and a one-ulp move of a coordinate below 16 A (ulp <= 9.5e-7) moves the atan2f operands by
    less than E1 (largest move in this set: 4.95e-6): |g| stays inside the margin on either side.  No edge is left out: every edge of the origin
    set that carries a torsion class is built, whatever else it flips.  On the ladders most rungs lie far outside the margin: fewer fallbacks
    than pairs proves that decisions next to a threshold were ACCEPTED and compared (the index bytes of those rungs equal the oracle's)."""
    import folddisco_amd as fd
    ctx, S = gpu
    _set_env(monkeypatch, {})
    es = S["origin"]
    idx = np.nonzero(np.array([any(str(c[0]).startswith("tor") for c in cl) for cl in es.classes]))[0]
    assert len(idx) >= 400
    X, aa = np.concatenate([es.XA[idx], es.XB[idx]]), np.concatenate([es.aa[idx], es.aa[idx]])
    d = qe.layout_per_pair(X, aa)
    batch = ctx.upload(qe.to_packed(d))
    ctx.spec_fallbacks()
    got = fd.FolddiscoIndex.build(ctx, batch).export()
    n_fb = ctx.spec_fallbacks()
    print(f"origin set: {len(idx)} torsion edges, fallbacks {n_fb} of {len(X)} pairs")
    oix, _, _ = oracle.build_index(qe.to_oracle_structs(d))
    _assert_index(got, oix, "origin torsion edges")
    assert n_fb == len(X)
    # ladders
    Xl, aal, celll, st = S["ladder"]
    for lname, dl in _layouts(Xl, aal, celll):
        batch = ctx.upload(qe.to_packed(dl))
        ctx.spec_fallbacks()
        got = fd.FolddiscoIndex.build(ctx, batch).export()
        n_fb = ctx.spec_fallbacks()
        print(f"ladder {lname}: fallbacks {n_fb} of {len(Xl)} pairs")
        oix, _, _ = oracle.build_index(qe.to_oracle_structs(dl))
        _assert_index(got, oix, f"ladder {lname}")
        assert 0 < n_fb < len(Xl)
    monkeypatch.setenv("FDGPU_EXACT", "1")
    ctx.spec_fallbacks()
    fd.FolddiscoIndex.build(ctx, batch)
    assert ctx.spec_fallbacks() == 0


def _assert_query_map(m, om):
    assert np.array_equal(m.hash, om["hash"]) and np.array_equal(m.qi, om["qi"]) and np.array_equal(m.qj, om["qj"])
    assert np.array_equal(m.is_primary, om["is_primary"]) and np.array_equal(m.idf.view(np.uint32), om["idf"].view(np.uint32))


def _assert_counts(got, want):
    assert [(r["nid"], r["total_match_count"], r["node_count"], r["edge_count"]) for r in got] == \
           [(r["nid"], r["total_match_count"], r["node_count"], r["edge_count"]) for r in want]
    for r, w in zip(got, want):
        assert r["idf"] == pytest.approx(w["idf"], rel=1e-5)


def _assert_retrieve(got, cand, ostructs, oq, om_, **okw):
    n = 0
    for slot, nid in enumerate(cand):
        R = oracle.retrieve(ostructs[int(nid)], oq, om_, **okw)
        mine = [g for g in got if g["cand"] == slot]
        assert len(mine) == len(R["processed"]), (int(nid), len(mine), len(R["processed"]))
        for g, rp, rh in zip(mine, R["processed"], R["from_hash"]):
            assert g["processed"] == [-1 if x is None else x[2] for x in rp["residues"]]
            assert g["from_hash"] == [-1 if x is None else x[2] for x in rh["residues"]]
            assert abs(g["rmsd"] - rp["rmsd"]) <= 1e-4 and g["idf"] == pytest.approx(rp["idf"], rel=1e-6)
            n += 1
    return n


def _item(d, s):
    a, b = int(d["res_off"][s]), int(d["res_off"][s + 1])
    return dict(n_xyz=d["n_xyz"][a:b], ca_xyz=d["ca_xyz"][a:b], cb_xyz=d["cb_xyz"][a:b], aa=d["aa"][a:b], cb_ok=None if d.get("cb_ok") is None else d["cb_ok"][a:b])


def test_query_side_on_packed_edges(gpu, monkeypatch):
    """make_query_map (threshold expansion; host form and both device forms), count_query and retrieve with packed edge structures as query
    and as candidates: all as the oracle computes them"""
    import folddisco_amd as fd
    from folddisco_amd import query as fq
    ctx, S = gpu
    _set_env(monkeypatch, {})
    X, aa, cell = S["default"].sides()
    d = qe.layout_packed(X, aa, cell)
    n_s = len(d["res_off"]) - 1
    half = n_s // 2                                   # structure s holds the A sides, s + half the B sides of the same edges
    batch = ctx.upload(qe.to_packed(d))
    ix = fd.FolddiscoIndex.build(ctx, batch)
    ostructs = qe.to_oracle_structs(d)
    oix, onres, _ = oracle.build_index(ostructs)
    pen = fd.length_penalty(onres, 0.5)
    n_match = 0
    for s, res in ((0, list(range(8))), (3, [10, 11, 40, 41, 90, 91]), (half + 1, list(range(100, 112))), (n_s - 1, [0, 1, 126, 127])):
        qb = ctx.upload(fd.PackedStructures.concat([_item(d, s)]))
        qstr = ",".join(f"A{i + 1}" for i in res)
        for dist_thr, angle_thr in (((0.5,), (5.0,)), ((0.5, 1.0), (5.0, 10.0))):
            om_ = oracle.make_query_map(ostructs[s], qstr, oix, float(n_s), dist_thr=dist_thr, angle_thr=angle_thr)
            om = om_.arrays()
            for mode in ("0", "1", "2"):
                monkeypatch.setenv("FDGPU_QM_DEVICE", mode)
                m = fq.make_query_map(ctx, qb, res, None, ix, float(n_s), dist_thr=dist_thr, angle_thr=angle_thr)
                _assert_query_map(m, om)
            monkeypatch.delenv("FDGPU_QM_DEVICE")
            m = fq.make_query_map(ctx, qb, res, None, ix, float(n_s), dist_thr=dist_thr, angle_thr=angle_thr)      # the default form
            _assert_query_map(m, om)
            _assert_counts(fd.count_query(ctx, ix, m.hash, m.qi, m.qj, pen, total_structures=n_s), oracle.count_query(om_, oix, onres))
            cand = np.array(sorted({s, (s + half) % n_s, (s + 1) % n_s}), np.uint32)
            got = fq.retrieve(ctx, batch, None, cand, m, qb)
            n_match += _assert_retrieve(got, cand, ostructs, ostructs[s], om_)
    assert n_match >= 8


_ser_cache = {}


def _cutoff_database(S, htype, cutoff):
    """the serine peptidases + a synthetic batch + the encoding's cutoff edges (both sides, one structure per pair) as one layout"""
    from folddisco_amd import synth
    if "ser" not in _ser_cache:
        ps, _ = oracle_structs_to_packed([oracle.read_pdb(p) for p in SER])
        sy = synth.to_packed(synth.generate(12, seed=4242))
        _ser_cache["ser"] = (ps, sy)
    ps, sy = _ser_cache["ser"]
    es = S["cutoff"][(htype, cutoff)]
    X, aa, _ = es.sides()
    e = qe.layout_per_pair(X, aa)
    parts = [dict(res_off=p.res_off, n_xyz=p.n_xyz, ca_xyz=p.ca_xyz, cb_xyz=p.cb_xyz, aa=p.aa, cb_ok=p.cb_valid) for p in (ps, sy)] + [e]
    off = [np.zeros(1, np.uint64)]
    for p in parts:
        off.append(p["res_off"][1:].astype(np.uint64) + off[-1][-1])
    return dict(res_off=np.concatenate(off), n_xyz=np.concatenate([p["n_xyz"] for p in parts]), ca_xyz=np.concatenate([p["ca_xyz"] for p in parts]),
                cb_xyz=np.concatenate([p["cb_xyz"] for p in parts]), aa=np.concatenate([p["aa"] for p in parts]),
                cb_ok=np.concatenate([np.ones(len(p["aa"]), np.uint8) if p.get("cb_ok") is None else p["cb_ok"] for p in parts])), es.cfg


@pytest.mark.parametrize("cutoff", [6.0, 12.5, 25.0])
@pytest.mark.parametrize("htype", [3, 2, 4, 5, 6])
def test_non_default_cutoffs_match_oracle(gpu, monkeypatch, htype, cutoff):
    """dist_cutoff away from 20: S1 lists, index bytes, query map, count records and matches equal the oracle's with the same cutoff, for the
    default encoding and one encoding per branch of fd_accept_other"""
    import folddisco_amd as fd
    from folddisco_amd import query as fq
    ctx, S = gpu
    _set_env(monkeypatch, {})
    d, cfg = _cutoff_database(S, htype, cutoff)
    n_s = len(d["res_off"]) - 1
    _assert_s1(ctx, d, cfg, cfg.name)
    batch = ctx.upload(qe.to_packed(d))
    ix = fd.FolddiscoIndex.build(ctx, batch, dist_cutoff=cutoff, hash_type=htype)
    ostructs = qe.to_oracle_structs(d)
    with oracle.hash_type(htype):
        oix, onres, _ = oracle.build_index(ostructs, cutoff=cutoff)
        _assert_index(ix.export(), oix, cfg.name)
        if htype == 3 and cutoff == 25.0:      # CA bins beyond 15 really occur
            # the accepted sides of the cutoff edges have d_CA = 25 A: CA bin 19 = 0b10011, OR-ed unmasked at bit 16, so bit 20 (the
            # lowest bit of the second residue type) is set by the CA field; checked on the DEVICE's raw lists where that type is even
            e0 = n_s - 2 * len(S["cutoff"][(htype, cutoff)])
            h, off = fd.get_geometric_hash_as_u32(ctx, batch, dist_cutoff=cutoff, sort_dedup=False)
            n_hi = 0
            for s in range(e0, n_s):
                a = int(off[s])
                if int(off[s + 1]) - a == 2 and d["aa"][int(d["res_off"][s]) + 1] % 2 == 0:
                    assert (int(h[a]) >> 16) & 0x1f == 19 and (int(h[a]) >> 25) == int(d["aa"][int(d["res_off"][s])]), s
                    n_hi += 1
            assert n_hi >= 16
            # the distance table's clamp (guess beyond bin 31, d > ~39 A) is not reached by these sets: see test_distance_table_clamp_takes_the_exact_path
        pen = fd.length_penalty(onres, 0.5)
        n_match = 0
        n_ser = len(SER)
        # a motif of a real structure, a motif of a synthetic one, and a cutoff edge structure itself
        for s, res in ((4, [60, 61, 62, 100, 150]), (n_ser + 2, [5, 6, 7, 30, 31]), (n_s - 3, list(range(cfg.nres)))):
            qb = ctx.upload(fd.PackedStructures.concat([_item(d, s)]))
            qstr = ",".join(f"A{i + 1}" for i in res)
            om_ = oracle.make_query_map(ostructs[s], qstr, oix, float(n_s), cutoff=cutoff)
            m = fq.make_query_map(ctx, qb, res, None, ix, float(n_s), dist_cutoff=cutoff, hash_type=htype)
            _assert_query_map(m, om_.arrays())
            want = oracle.count_query(om_, oix, onres)
            _assert_counts(fd.count_query(ctx, ix, m.hash, m.qi, m.qj, pen, total_structures=n_s), want)
            cand = np.array(sorted({s, 0, n_ser + 2, n_s - 3, n_s - 3 - len(S["cutoff"][(htype, cutoff)])}), np.uint32)
            got = fq.retrieve(ctx, batch, None, cand, m, qb, dist_cutoff=cutoff, hash_type=htype)
            n_match += _assert_retrieve(got, cand, ostructs, ostructs[s], om_, cutoff=cutoff)
        assert n_match >= 2


def test_cli_grid_width_round_trip(gpu, tmp_path):
    """`index -g 12.5` writes grid_width into PREFIX.type, `query` reads it back: index files equal the oracle's for that cutoff, the rows equal
    those of the in-process query with dist_cutoff=12.5 and every row's residues are a match the oracle reports for that cutoff (each CLI
    process opens the device under its own time limit; the in-process part uses the module's context)"""
    import folddisco_amd as fd
    ctx, _ = gpu
    from folddisco_amd import indexio
    from folddisco_amd import query as fq
    from folddisco_amd import structure as st
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    for k in ("FDGPU_DTAB", "FDGPU_EXACT", "FDGPU_MSD", "FDGPU_QM_DEVICE"):
        env.pop(k, None)
    pre = str(tmp_path / "ix")
    subprocess.run([sys.executable, "-m", "folddisco_amd", "index", "-p", os.path.dirname(SER[0]), "-i", pre, "-g", "12.5"], env=env, check=True, timeout=300)
    assert indexio.load_type(pre + ".type")["grid_width"] == 12.5
    ostructs = [oracle.read_pdb(p) for p in SER]
    oix, onres, _ = oracle.build_index(ostructs, cutoff=12.5)
    v, h, o = indexio.read_index_files(pre)
    assert np.array_equal(h, oix.hashes()) and np.array_equal(o, oix.offsets()) and np.array_equal(v, oix.values())
    o20, _, _ = oracle.build_index(ostructs)
    assert oix.H < o20.H
    out = str(tmp_path / "out.tsv")
    subprocess.run([sys.executable, "-m", "folddisco_amd", "query", "-p", Q4CHA, "-q", "B57,B102,C195", "-i", pre, "-o", out], env=env, check=True, timeout=300)
    rows = [l.rstrip("\n").split("\t") for l in open(out)]
    structs = [st.read_compact_structure(p) for p in SER]
    batch = ctx.upload(fd.PackedStructures.concat([s.as_item() for s in structs]))
    ix = fd.FolddiscoIndex.build(ctx, batch, dist_cutoff=12.5)
    nres = np.array([s.n for s in structs], np.uint64)
    plddt = np.array([s.avg_plddt() for s in structs], np.float32)
    q = st.read_compact_structure(Q4CHA)
    _, want = fq.query_pdb(ctx, ix, batch, structs, list(SER), nres, plddt, q, "B57,B102,C195", dist_cutoff=12.5, sort_by="")
    assert [r[1:] for r in rows] == [fq.format_match_row(m).split("\t")[1:] for m in want] and len(rows) >= 3
    oq = oracle.read_pdb(Q4CHA)
    om_ = oracle.make_query_map(oq, "B57,B102,C195", oix, 5.0, cutoff=12.5)
    omatches = set()
    for k, p in enumerate(SER):
        for mt in oracle.retrieve(ostructs[k], oq, om_, cutoff=12.5)["processed"]:
            omatches.add((os.path.basename(p), ",".join("_" if x is None else f"{x[0]}{x[1]}" for x in mt["residues"])))
    for r in rows:
        assert (os.path.basename(r[0]), r[4]) in omatches, r


def test_distance_table_clamp_takes_the_exact_path(gpu, monkeypatch):
    """A squared distance whose v_sqrt_f32 guess lies beyond the table (bin > 31: d above 2 + 31.5 * 1.2 = 39.8 A) clears `ok` in fd_dist_bin_tab
    and the pair takes the exact routine.  Reached with a 45 A cutoff: 192 pairs with d_CA in 36..44.5 A; index bytes equal the oracle's and
    every pair with d_CA above 40 A is counted as a fallback."""
    import folddisco_amd as fd
    ctx, _ = gpu
    _set_env(monkeypatch, {})
    X, aa, dist = qe.far_pairs(192, 36.0, 44.5, seed=4545)
    d = qe.layout_per_pair(X, aa)
    batch = ctx.upload(qe.to_packed(d))
    ctx.spec_fallbacks()
    got = fd.FolddiscoIndex.build(ctx, batch, dist_cutoff=45.0).export()
    n_fb = ctx.spec_fallbacks()
    oix, _, _ = oracle.build_index(qe.to_oracle_structs(d), cutoff=45.0)
    _assert_index(got, oix, "clamp")
    n_far = int((dist > 40.0).sum())
    print(f"clamp: {n_far} pairs beyond 40 A, fallbacks {n_fb}")
    assert oix.H >= 300 and n_far >= 64 and n_fb >= n_far
