"""The hand-made scoring cases of scoring_cases.py on the host: the generator is deterministic, every case class is there and every case has the property
it claims under the model (byte lengths on both sides of each stride threshold, straddled block and slot offsets, slot counts, the sums of the width
cases, tie counts against the selection's cap, kept rows), every list round-trips through the codec, and the model agrees with the oracle's
count_query on every case with first_id = 0 except the shard view (free (node, edge) rows go in through a hand-filled fdo_query_map; the oracle
takes total_structures = the number of structures and penalty = nres^-0.5, so the model is run with those on the cases' lists and rows: counts equal,
idf within the pinned relative 1e-5 — the oracle sums f32 in its own order)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import scoring_cases as sc
from tests.helpers import Q4CHA

CAP = 50 + 1024          # what the device selection holds at the crowd cases' top_n = 50


@pytest.fixture(scope="module")
def maps():
    oq = oracle.read_pdb(Q4CHA)
    out = {}
    for name, motif in (("big", sc.MOTIF), ("small", sc.MOTIF_SMALL)):
        m = oracle.make_query_map(oq, motif, None, 0.0).arrays()
        out[name] = (m["hash"].astype(np.uint32), m["qi"].astype(np.uint32), m["qj"].astype(np.uint32))
    return out


@pytest.fixture(scope="module")
def slots(maps):
    return sc.map_slots(maps["big"][0], maps["small"][0])


def all_cases(first_id, slots):
    return sc.batch_cases(first_id) + sc.map_cases(first_id, slots[1])


def test_motif_is_the_shortest_run_with_160_entries(maps):
    """B18 .. B24: no run of fewer than seven consecutive residues of 4CHA reaches 160 map entries, and this is the first of seven that does"""
    oq = oracle.read_pdb(Q4CHA)
    a = oq.arrays()
    ch, se = a["chain"], a["serial"]
    first = None
    for n in range(2, 8):
        for s in range(oq.n - n + 1):
            if len(set(ch[s:s + n])) != 1 or int(se[s + n - 1]) - int(se[s]) != n - 1:
                continue
            q = "%s%d-%d" % (chr(ch[s]), int(se[s]), int(se[s + n - 1]))
            if len(oracle.make_query_map(oq, q, None, 0.0).arrays()["hash"]) >= 160:
                first = first or (n, q)
                break
        if first:
            break
    assert first == (7, sc.MOTIF)
    assert len(maps["big"][0]) == sc.MAX_MAP_ROWS == len(set(maps["big"][0].tolist()))
    assert len(maps["small"][0]) >= 5 and np.isin(maps["small"][0], maps["big"][0]).all()


def test_generator_is_deterministic_and_complete(slots):
    for f in sc.FIRST_IDS:
        a, b = all_cases(f, slots), all_cases(f, slots)
        assert [repr(c) for c in a] == [repr(c) for c in b]
        for x, y in zip(a, b):
            ix, iy = x.index(f, slots[0]), y.index(f, slots[0])
            assert all(np.array_equal(p, q) for p, q in zip(ix[:3], iy[:3]))
            assert np.array_equal(x.penalty.view(np.uint32), y.penalty.view(np.uint32)) and x.total == y.total and x.top_ns == y.top_ns
        for via in ("batch", "maps"):
            have = {c.cls for c in a if c.via == via}
            want = set(sc.CLASSES) - ({"groups"} if via == "maps" else set())          # (node, edge) are free only outside a map
            assert have == want, (f, via)
        assert all(len(c.lists) and len(c.queries) and c.claims for c in a)
    assert sc.S == 88101 and sc.NC == 44 and sc.NT == 6 and sc.S % 32
    assert sc.FIRST_IDS[3] + sc.S == 0xffffffff
    assert len(sc.varint(sc.FIRST_IDS[2])) == 4 and len(sc.varint(sc.FIRST_IDS[2] + sc.S - 1)) == 5
    assert [48 * ((sc.NC + (1 << j) - 1) >> j) for j in range(5, -1, -1)] == list(sc.STRIDE_THRESHOLDS)


def _sums32(fixes_per_query, rows_per_query):
    """what the dispatch asks of a batch before it sums in 32 bits: no row of zero units, every query's units below 2^32, at most 128 rows"""
    return all(int(f.min(initial=1)) != 0 and sum(int(x) for x in f) < 1 << 32 for f in fixes_per_query) and max(rows_per_query) <= 128


def check_claims(c, f, L, rows):
    cl = c.claims
    A = c.abs_lists(f)
    mods = [sc.model_full(L, q, c.total, c.penalty, f, sc.S) for q in rows]
    kept = [m[3][m[2] > 0] for m in mods]
    if "bytes" in cl:
        assert [sc.list_bytes(a) for a in A] == cl["bytes"]
        js = [sc.qt_stride(n)[0] for n in cl["bytes"]]
        assert all(js[k] == js[k + 1] + 1 for k in range(0, len(js), 2)) and sorted(set(js)) == list(range(7))
        assert all(set((a - f) >> sc.TILE_LOG2) == set(range(sc.NT)) for a in A)
    if "dense" in cl:
        assert np.array_equal(A[cl["dense"]] - f, np.arange(sc.S)) and sc.list_bytes(A[cl["dense"]]) == sc.S - 1 + len(sc.varint(f))
    if "empty_tiles" in cl:
        assert [sorted(set(range(sc.NT)) - set(((a - f) >> sc.TILE_LOG2).tolist())) for a in A] == cl["empty_tiles"]
        assert any(sc.qt_stride(sc.list_bytes(a))[0] == 0 for a in A) and any(sc.qt_stride(sc.list_bytes(a))[0] > 0 for a in A)
    if "single" in cl:
        assert [(a - f).tolist() for a in A] == [[x] for x in cl["single"]]
    if "straddle64" in cl:
        for a, (w, before) in zip(A, cl["straddle64"]):
            assert (w, before, True) in sc.straddles(a, 64, f) and sc.qt_stride(sc.list_bytes(a))[0] == 0
        assert {w for w, _ in cl["straddle64"]} == ({2, 3, 5} if sc._can_step_2_28(f) else {2, 3})
    if "straddle16" in cl:
        for a, (w, before) in zip(A, cl["straddle16"]):
            assert (w, before) in {x[:2] for x in sc.straddles(a, 16, f)}
        assert {(w, b) for w, b in cl["straddle16"]} >= {(2, 1), (3, 1), (3, 2)} | ({(5, 1), (5, 2), (5, 3), (5, 4)} if sc._can_step_2_28(f) else set())
    if "slots" in cl:
        assert set(cl["slots"]) <= set(sc.slots_of(A[0], f))
    if "ends" in cl:
        for a, (n, wl) in zip(A, cl["ends"]):
            assert sc.list_bytes(a) == n < 96 and int(sc.varint_spans(a)[1][-1]) == wl and sc.slots_of(a, f) == [(n + 15) // 16]
        assert {n % 16 for n, _ in cl["ends"]} == {15, 0, 1}
    if "window_sums" in cl:
        for (li, _, _), want in zip(c.base_queries, cl["window_sums"]):
            sl = [sc.slots_of(A[int(k)], f) for k in li]
            assert all(len(x) == 1 for x in sl) and sum(x[0] for x in sl[:-1]) == want and sl[-1] == [2]
    if "tied" in cl:
        r = sc.rank(mods[0][0], 1 << 30)
        lo, hi = cl["above"], cl["above"] + cl["tied"][0]
        assert len({x.tobytes()[4:] for x in r[lo:hi]}) == 1 and (lo == 0 or r[lo - 1]["idf"] > r[lo]["idf"]) and r[hi]["idf"] < r[lo]["idf"]
        assert (c.penalty == 1.0).all() and any(lo < n < hi for n in c.top_ns) and np.array_equal(r[lo:hi]["nid"], np.sort(r[lo:hi]["nid"]))
        tiles = np.bincount((r[lo:hi]["nid"].astype(np.int64) - f) >> sc.TILE_LOG2)
        assert (tiles > 0).sum() >= 2
        if "per_tile" in cl:
            assert tuple(tiles[tiles > 0]) == cl["per_tile"] and set(cl["per_tile"]) <= set(c.top_ns)
    if "crowd" in cl:
        K = cl["crowd"]
        r = sc.rank(mods[0][0], 1 << 30)
        keys = [sc.order_key(x) for x in r["idf"][:K + 2]]
        assert max(keys[:K]) - min(keys[:K]) == (0 if not cl["ulp"] else max(keys[:K]) - min(keys[:K])) <= 2 and (len(set(keys[:K])) == 2) == cl["ulp"]
        assert len({(sc.key_bin(k), sc.sub_bin(k)) for k in keys[:K]}) == 1
        assert sc.key_bin(keys[K]) == sc.key_bin(keys[0]) != sc.key_bin(keys[K + 1]) and sc.sub_bin(keys[K]) != sc.sub_bin(keys[0])
        # the first level sees K + 1 keys in the cut's bin (second level when that exceeds the cap), the second K in its sub-bin (overflow when that does)
        assert (K + 1 > CAP) == (K >= 1074) and (K > CAP) == cl["overflow"] and c.top_ns == (50,)
    if "cut_bin" in cl:
        r = sc.rank(mods[0][0], 1 << 30)
        assert sc.key_bin(sc.order_key(r["idf"][49])) == cl["cut_bin"]
        if cl["cut_bin"] == 0:
            z = sc.order_key(0.0)
            ks = [sc.order_key(x) for x in r["idf"]]
            assert sum(k > z for k in ks) < 50 and sum(k == z for k in ks) >= 3000 and sum(k < z for k in ks) >= 10
            assert (r["idf"].view(np.uint32) == 0x80000000).any()          # -0 among them
        else:
            assert float(r["idf"][49]) > 65536.0
    if "sum_at" in cl:
        full, sums = mods[0][0], mods[0][1]
        s = sums[int(np.flatnonzero(full["nid"] == f + cl["sum_at"])[0])]
        assert cl["sum_lo"] <= s < cl["sum_hi"] and len(kept[0]) == 34
        if cl["sums32"]:
            assert s == max(sums) == (1 << 32) - 184          # with libm's log2f(2^31 / 32769); the bound asked for is [2^32 - 2^12, 2^32)
    if "sums32" in cl:
        assert _sums32(kept, [len(k) for k in kept]) == cl["sums32"]
    if "zero_unit_row" in cl:
        full, sums = mods[0][0], mods[0][1]
        assert 0 in [int(x) for x in kept[0]]
        assert sum(1 for x, s in zip(full, sums) if s == 0 and x["total_match_count"] == 1) == cl["only_zero"] and len(full) == sc.S
    if "min_fix" in cl:
        assert max(int(x) for x in kept[0]) >= cl["min_fix"]
    if "kept" in cl:
        assert [len(k) for k in kept] == cl["kept"]
    if "group_ends" in cl:
        li, node, edge = (np.asarray(x) for x in c.queries[0])
        o = np.lexsort((edge, node))          # stable
        gk = node[o] * 4 + edge[o]
        ends = set(np.flatnonzero(np.concatenate([gk[1:] != gk[:-1], [True]])).tolist())
        assert set(cl["group_ends"]) <= ends and not ends & set(range(cl["span"][0], cl["span"][1])) and cl["span"][1] in ends and len(ends) == cl["n_groups"]
        assert not (np.diff(node) >= 0).all()          # given out of order
        full = mods[0][0]
        x1, x2, x3 = (full[full["nid"] == f + x][0] for x in cl["X"])
        assert (int(x1["total_match_count"]), int(x1["edge_count"])) == (2, 1) and (int(x2["total_match_count"]), int(x2["edge_count"])) == (1, 1)
        assert int(x3["edge_count"]) == cl["n_groups"] and int(x3["node_count"]) == len(set(node.tolist()))
        rows_x1 = [k for k in range(len(o)) if cl["X"][0] + f in L[int(rows[0][0][o[k]])]]
        rows_x2 = [k for k in range(len(o)) if cl["X"][1] + f in L[int(rows[0][0][o[k]])]]
        assert not set(rows_x1) & ends and set(rows_x2) <= ends
        assert len(set(np.asarray(c.queries[1][1]).tolist())) == 1 and len(set(np.asarray(c.queries[2][1]).tolist())) == len(c.queries[2][1])
    if "outside" in cl:
        for k in cl["outside"]:
            assert not ((A[k] >= f) & (A[k] < f + sc.S)).any()
        assert any(((a < f).any() and (a >= f).any()) for a in A) or f == 0
        assert any(((a >= f + sc.S).any() and (a < f + sc.S).any()) for a in A)


@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_every_case_has_the_property_it_claims(first_id, maps, slots):
    seen = set()
    for c in all_cases(first_id, slots):
        h, o, v, L = c.index(first_id, slots[0])
        assert (np.diff(h.astype(np.int64)) > 0).all() and int(o[-1]) == len(v)
        for k in range(len(h)):          # every list round-trips through the codec
            assert sc.decode(bytes(v[int(o[k]):int(o[k + 1])])) == L[int(h[k])].tolist()
        if c.in_range:
            assert all(((a >= first_id) & (a < first_id + sc.S)).all() for a in L.values())
        rows = c.rows(maps)
        assert all(len(q[0]) for q in rows)
        check_claims(c, first_id, L, rows)
        seen.add((c.cls, c.via))
    assert {x[0] for x in seen} == set(sc.CLASSES)


class _Rows:
    """(hash, node, edge_j) rows as the fdo_query_map the oracle's count_query reads (it uses n, hash, qi and qj only)"""

    def __init__(self, q):
        self.keep = (np.ascontiguousarray(q[0], np.uint32), np.ascontiguousarray(q[1], np.uint64), np.ascontiguousarray(q[2], np.uint64))
        h, n, e = self.keep
        self.m = oracle.QueryMap(n=len(h), hash=h.ctypes.data_as(oracle.u32p), qi=n.ctypes.data_as(oracle.u64p), qj=e.ctypes.data_as(oracle.u64p))
        self.ptr = C.pointer(self.m)


def test_model_equals_oracle_on_every_case_at_first_id_0(maps, slots):
    libm = C.CDLL("libm.so.6")
    libm.powf.restype = C.c_float
    libm.powf.argtypes = [C.c_float, C.c_float]
    nres = (50 + (np.arange(sc.S, dtype=np.int64) * 7919) % 900).astype(np.uint64)
    lut = {int(n): libm.powf(float(n), -0.5) for n in np.unique(nres)}
    pen = np.array([lut[int(n)] for n in nres], np.float32)
    compared = set()
    worst = 0.0
    for c in all_cases(0, slots):
        if c.cls == "shard":
            continue
        h, o, v, L = c.index(0, slots[0])
        oix = oracle.BorrowedIndex(h, o, v)
        for q in c.rows(maps):
            want = oracle.count_query(_Rows(q), oix, nres)
            got = sc.model_full(L, q, sc.S, pen, 0, sc.S)[0]
            assert len(got) == len(want) > 0, c
            for key in ("nid", "total_match_count", "node_count", "edge_count"):
                assert np.array_equal(got[key], np.array([w[key] for w in want], np.uint32)), (c, key)
            w_idf = np.array([w["idf"] for w in want], np.float64)
            rel = np.abs(got["idf"].astype(np.float64) - w_idf) / np.maximum(np.abs(w_idf), 1e-30)
            rel[(w_idf == 0) & (got["idf"] == 0)] = 0.0
            worst = max(worst, float(rel.max()))
            assert rel.max() <= 1e-5, (c, float(rel.max()))
        compared.add((c.cls, c.via))
    print("largest relative idf difference, model vs oracle:", worst)
    assert {x[0] for x in compared} == set(sc.CLASSES) - {"shard"}
