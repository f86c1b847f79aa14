"""The hand-made retrieval cases of retrieval_cases.py on the CPU: every case's claims against the oracle's own found / cand / match output and against
the module's Python model of the glue (which the same tests pin to the oracle), and every threshold a class names with a case on each side of it.
A case whose claim does not hold is a broken case: it fails here, it is never left out of the GPU module."""
import numpy as np
import pytest

import oracle
from tests import retrieval_cases as rc


def _res(m):
    return [-1 if x is None else x[2] for x in m["residues"]]


def _model(c, k=0):
    T = c.targets[k]
    found, cand = rc.model_scan(T, c.arrays, c.ca_distance_cutoff)
    return found, cand, rc.model_glue(found, cand, c.arrays, c.node_count)


@pytest.mark.parametrize("cls", rc.CLASSES)
def test_model_equals_oracle(cls):
    """pair scan, component order, mappings, rescue and idf of the Python model == the oracle, for every target of every case, exactly"""
    for c in rc.cases(cls):
        for k, R in enumerate(rc.oracle_results(c)):
            found, cand, g = _model(c, k)
            assert np.array_equal(found, R["found"]) and np.array_equal(cand, R["cand"]), (c, k)
            assert len(g["records"]) == len(R["from_hash"]), (c, k)
            for rec, fh, pr in zip(g["records"], R["from_hash"], R["processed"]):
                assert rec["from_hash"] == _res(fh) and rec["processed"] == _res(pr), (c, k)
                assert np.float32(fh["idf"]).view(np.uint32) == np.float32(rec["idf"]).view(np.uint32) and fh["idf"] == pr["idf"], (c, k)


@pytest.mark.parametrize("cls", rc.CLASSES)
def test_claims_hold(cls):
    cs = rc.cases(cls)
    assert cs
    for c in cs:
        R = rc.oracle_results(c)[0]
        found, cand, g = _model(c)
        recs, cl, a = g["records"], c.claims, c.arrays
        n_nodes = len(set(R["found"][:, 0].tolist()) | set(R["found"][:, 1].tolist()))
        assert n_nodes == len(g["nodes"])
        got = dict(F=len(R["found"]), nodes=n_nodes, C=len(R["cand"]), comps=len(R["from_hash"]), n_components=len(R["from_hash"]), hashes=len(np.unique(a["hash"])),
                   entries=len(a["hash"]), n_indices=len(a["indices"]), n_aad=len(a["aad_dist"]), residues=c.targets[0].n)
        for key in got:
            if key in cl:
                assert got[key] == cl[key], (c, key, got[key])
        if "max_nodes" in cl:
            assert n_nodes <= cl["max_nodes"], c
        if "min_comps" in cl:
            assert len(recs) >= cl["min_comps"], c
        if "components" in cl:
            assert g["comps"] == cl["components"], (c, g["comps"])
        if "comp_sizes" in cl:
            assert [len(x) for x in g["comps"]] == cl["comp_sizes"], c
        if "last_node_in" in cl:
            assert [len(x) for x in g["comps"] if n_nodes - 1 in x] == cl["last_node_in"], c
        for flag in ("tie", "skipped", "stopped", "quirk", "quirk_other"):
            if flag in cl:
                assert recs[0][flag] == cl[flag], (c, flag)
        if "mapping" in cl:
            assert [dict(r["assigned"]) for r in recs[:len(cl["mapping"])]] == cl["mapping"], (c, [r["assigned"] for r in recs])
            for r, fh in zip(recs, R["from_hash"]):          # the oracle's from-hash list says the same
                want = [dict(r["assigned"]).get(int(q), -1) for q in a["indices"]]
                assert _res(fh) == want, c
        if "symmetric" in cl:
            assert sum(bool(oracle.lib().fdo_hash_is_symmetric(int(h))) for h in np.unique(a["hash"])) == cl["symmetric"], c
            assert any(oracle.lib().fdo_hash_is_symmetric(int(h)) for h in R["found"][:, 2]) and not all(oracle.lib().fdo_hash_is_symmetric(int(h)) for h in R["found"][:, 2]), c
        if "quirk" in cl and cl["quirk"]:
            assert len(set(a["indices"].tolist())) < len(a["indices"]), c
        if "tally" in cl:
            pos = len(a["indices"]) - 1          # the unmatched query residue stands last
            assert recs[0]["from_hash"][pos] == -1 and recs[0]["tallies"].get(pos) == cl["tally"], (c, recs[0]["tallies"])
        if "rescued" in cl:
            fh, pr = _res(R["from_hash"][0]), _res(R["processed"][0])
            assert bool(recs[0]["rescued"]) == cl["rescued"] and (fh != pr) == cl["rescued"], (c, recs[0]["tallies"])
            if cl["rescued"]:
                assert all(fh[p] == -1 and pr[p] >= 0 for p in recs[0]["rescued"]), c
        if "rescue_row_from" in cl:          # the winner's votes reach into the last 64 candidate pairs that the LDS copy holds
            pos = recs[0]["rescued"][0]
            rows = np.flatnonzero((R["cand"][:, 0] == int(a["indices"][pos])) & (R["cand"][:, 1] == recs[0]["processed"][pos]))
            assert len(rows) >= 4 and rows.max() >= cl["rescue_row_from"], (c, rows)
        if "filt" in cl:
            assert recs[0]["filt"] == cl["filt"], (c, recs[0]["filt"])
        if "tags_passing" in cl:
            i, j = cl["pair"]
            rows = R["cand"][(R["cand"][:, 1] == i) & (R["cand"][:, 2] == j)]
            assert sorted(rows[:, 0].tolist()) == cl["tags_passing"], (c, rows)
        if "tags_absent" in cl:
            assert not np.isin(R["cand"][:, 0], cl["tags_absent"]).any(), c
        for key in ("q_residues", "tally_len", "max_vote", "sat_winner"):
            if key in cl:
                assert max(r[key] for r in recs) == cl[key], (c, key, [r[key] for r in recs])
        if "min_filt" in cl:          # the split form takes the unfiltered walk
            assert recs[0]["filt"] >= cl["min_filt"], (c, recs[0]["filt"])
        if "winner" in cl:          # the saturated tie goes to the smaller residue, in the model and in the oracle's from-hash list
            sat = [k for k, r in enumerate(recs) if r["max_vote"] == 255 and r["sat_winner"]]
            assert sat and all(cl["winner"] in recs[k]["assigned"] for k in sat), c
            pos = a["indices"].tolist().index(cl["winner"][0])
            assert all(_res(R["from_hash"][k])[pos] == cl["winner"][1] for k in sat), c
        # the way the call goes, restated from the limits of the two forms of the device glue, over every candidate of the call
        over_split, over_slots = False, False
        for k in range(len(c.targets)):
            fk, _, gk = (found, cand, g) if k == 0 else _model(c, k)
            hard = len(gk["nodes"]) > rc.WAVE or len(fk) > rc.RS_EDGE_CAP or any(r["q_residues"] > rc.WAVE for r in gk["records"])
            slots = hard or any(r["tally_len"] > rc.RS_LIST_CAP for r in gk["records"])
            # the split form keeps a slot of at most RS_S_EDGE found triples; its rescue list overflows only in the unfiltered walk
            split = slots if len(fk) > rc.RS_S_EDGE else hard or any(r["filt"] > rc.RS_S_FILT and r["tally_len"] > rc.RS_S_LIST for r in gk["records"])
            over_split, over_slots = over_split or split, over_slots or slots
        assert over_split or not over_slots, c
        host = len(a["indices"]) > rc.WAVE or len(a["aad_dist"]) > rc.TWO_PASS_AAD
        assert c.path == ("host" if host else "overflow" if over_split else "device"), c
        assert c.split_only == (not host and over_split and not over_slots), c
        if c.path == "device":          # none of the list caps is met by accident
            assert len(recs) <= 2 * rc.WAVE and all(r["votes"] <= 2 * min(len(found), rc.RS_S_EDGE) and r["max_vote"] < 255 for r in recs), c          # (two votes per found triple at most: the vote lists' caps are out of reach)
            assert int(max(a["qi"].max(), a["qj"].max())) < c.query.n
        for k in range(1, len(c.targets) if "max_vote" not in cl else 1):          # (the saturation case: 150 nodes in both)  the ordinary candidate beside it stays inside every hard limit, and below the split form's hand-over
            Rk = rc.oracle_results(c)[k]
            assert len(set(Rk["found"][:, 0].tolist()) | set(Rk["found"][:, 1].tolist())) <= rc.WAVE and len(Rk["found"]) <= rc.RS_EDGE_CAP, c
            if c.name in ("F%d" % rc.RS_S_EDGE, "F%d" % (rc.RS_S_EDGE + 1)):
                assert 0 < len(Rk["found"]) <= rc.RS_S_EDGE, c


THRESHOLDS = (          # class, threshold, the quantity read from the oracle's output of the first candidate (or from the map)
    ("nodes", rc.WAVE, lambda c, R, g: len(g["nodes"])),
    ("edges", rc.RS_S_EDGE, lambda c, R, g: len(R["found"])),
    ("edges", rc.RS_EDGE_CAP, lambda c, R, g: len(R["found"])),
    ("comps", rc.WAVE, lambda c, R, g: len(R["from_hash"])),
    ("rescue", rc.RS_CAND_LDS, lambda c, R, g: len(R["cand"])),
    ("rescue", rc.RS_S_FILT, lambda c, R, g: g["records"][0]["filt"] if g["records"] else 0),
    ("sizes", rc.WAVE, lambda c, R, g: len(c.arrays["indices"])),
    ("rescue", rc.RS_S_LIST, lambda c, R, g: max([r["tally_len"] for r in g["records"]], default=0)),
    ("rescue", rc.RS_LIST_CAP, lambda c, R, g: max([r["tally_len"] for r in g["records"]], default=0)),
    ("votes", rc.WAVE, lambda c, R, g: max([r["q_residues"] for r in g["records"]], default=0)),
    ("sizes", rc.PREFILTER, lambda c, R, g: len(np.unique(c.arrays["hash"]))),
    ("sizes", rc.SETUP_HASH_LDS, lambda c, R, g: len(np.unique(c.arrays["hash"]))),
    ("sizes", rc.MP_QH_LDS, lambda c, R, g: len(np.unique(c.arrays["hash"]))),
    ("sizes", rc.RS_LIST_CAP, lambda c, R, g: len(np.unique(c.arrays["hash"]))),
    ("sizes", rc.AAD_SORTED, lambda c, R, g: len(c.arrays["aad_dist"])),
    ("sizes", rc.MP_AAD_LDS, lambda c, R, g: len(c.arrays["aad_dist"])),
    ("sizes", rc.TWO_PASS_AAD, lambda c, R, g: len(c.arrays["aad_dist"])),
    ("long", 64 * rc.MP_SCAN_BLOCKS, lambda c, R, g: c.targets[0].n),
    ("votes", rc.HOST_DENSE, lambda c, R, g: len(R["found"])),          # the host glue's switches (fd_retrieve_host.cpp): dense vote table, hash -> entry table
    ("votes", rc.HOST_DENSE, lambda c, R, g: len(np.unique(c.arrays["hash"]))),
)


@pytest.mark.parametrize("k", range(len(THRESHOLDS)))
def test_both_sides_of_every_threshold(k):
    cls, thr, qty = THRESHOLDS[k]
    seen = {qty(c, rc.oracle_results(c)[0], _model(c)[2]) for c in rc.cases(cls)}
    if cls == "comps":          # more than 64 components in one slot (65 and 96) beside slots with a handful
        assert min(seen) <= thr and {thr + 1, 3 * thr // 2} <= seen, sorted(seen)
        return
    assert thr in seen and thr + 1 in seen, (cls, thr, sorted(seen))
    if cls in ("nodes", "edges", "rescue") or THRESHOLDS[k][1] == rc.WAVE and cls == "sizes":          # the limits with a case one below as well: nodes, found triples, candidate pairs, `indices`
        assert thr - 1 in seen, (cls, thr, sorted(seen))


def test_window_class_covers_its_forms():
    names = {c.name: c for c in rc.cases("window")}
    assert {"ulp_1", "ulp_1.5", "ulp_3", "cutoff_zero", "cutoff_nan", "residue_types", "merged_overlap", "merged_abut", "merged_gap_inside"} <= set(names)
    assert names["cutoff_zero"].ca_distance_cutoff == 0.0 and np.isnan(names["cutoff_nan"].ca_distance_cutoff)
    assert set(names["residue_types"].arrays["aad_aa1"].tolist()) >= {20, 32, 255} and set(names["residue_types"].arrays["aad_aa2"].tolist()) >= {31, 33, 255}
    for n in ("merged_overlap", "merged_abut", "merged_gap_inside"):
        assert len(names[n].arrays["aad_dist"]) > rc.MP_AAD_LDS


def test_component_order_is_list_order():
    """the independent witness of the component order: ascending node lists, sorted as lists, duplicates dropped — a prefix sorts first, whatever its size"""
    assert rc.component_order([{2, 3}, {0, 1, 2, 3}, {1, 0}, {0, 1}]) == [[0, 1], [0, 1, 2, 3], [2, 3]]
    assert rc.component_order([{1, 2}, {0, 1, 2}]) == [[0, 1, 2], [1, 2]]
    assert rc.component_order([{0}, {1}, {0, 1}, {63}, {0, 63}]) == [[0], [0, 1], [0, 63], [1], [63]]
    for cls in ("comps", "nodes"):          # and the oracle's records follow it: a record's mapped residues are residues of its component
        for c in rc.cases(cls):
            R = rc.oracle_results(c)[0]
            _, _, g = _model(c)
            assert len(g["comps"]) == len(R["from_hash"])
            for comp, fh in zip(g["comps"], R["from_hash"]):
                assert {x for x in _res(fh) if x >= 0} <= {g["nodes"][v] for v in comp}, c


def test_maps_round_trip():
    """the two hand-made structs hold the arrays they were made from"""
    c = rc.cases("votes")[0]
    m = rc.oracle_map(c.arrays)
    s = m.ptr.contents
    assert s.n == len(c.arrays["hash"]) and [s.hash[k] for k in range(s.n)] == c.arrays["hash"].tolist() and [s.indices[k] for k in range(s.n_indices)] == c.arrays["indices"].tolist()
    q = rc.library_map(c.arrays)
    assert q.ctx is None and np.array_equal(q.indices, c.arrays["indices"]) and np.array_equal(q.hash, c.arrays["hash"]) and np.array_equal(q.primary_hash, c.arrays["hash"])
    assert np.array_equal(q.aad_dist.view(np.uint32), c.arrays["aad_dist"].view(np.uint32)) and np.array_equal(q.idf, c.arrays["idf"])
    h = q.handle.contents
    assert not h.post_len and not h.post_seg and not h.post_kidx and h.post_index_uid == 0 and h.arena_bytes == 0
