"""The pair scan's host block (csrc/fd_match_tables.cpp, through fdgpu_debug_match_tables) on the CPU: start tables and group order on both sides of the
256-entry switch between their two construction paths, the merged float intervals of queries with more than 1,024 observed distances probed at every end,
the work items in both forms at the switches of j_span, the hash-set slots, the layout.  Every witness is numpy written here; no device is opened."""
import ctypes as C

import numpy as np
import pytest

from folddisco_amd import _lib

LAYOUT = ("cand", "wc", "wi", "wq", "wj", "hashes", "start", "dist", "qi", "qtab", "iv_start", "iv", "iv_grp", "wbase", "cq", "words")
QTAB = ("qh_off", "n_hashes", "aad_off", "n_aad", "aa1_mask", "aa2_mask", "use_prefilter", "ca_window", "qs_off", "qs_mask")      # mp_query_dev, a word each
EINVAL, ERANGE = -1, -4
_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]
f32 = np.float32


def query(hashes=(), aa1=(), aa2=(), dist=(), qi=None, window=1.0, prefilter=1):
    n = len(dist)
    return dict(hashes=np.ascontiguousarray(hashes, np.uint32), aa1=np.ascontiguousarray(aa1, np.uint8), aa2=np.ascontiguousarray(aa2, np.uint8),
                dist=np.ascontiguousarray(dist, np.float32), qi=np.arange(n, dtype=np.uint32) if qi is None else np.ascontiguousarray(qi, np.uint32),
                window=window, prefilter=prefilter)


def build(queries, cands, lens, dev_items, pooled=0, hash_type=3):
    """queries: query() dicts; cands: per query the structure ids it scans; lens: residues per structure of the batch -> the entry's outputs"""
    qs = (_lib.MatchQuery * max(len(queries), 1))()
    for s, q in zip(qs, queries):
        s.hashes, s.n_hashes = q["hashes"].ctypes.data_as(_lib.u32p), len(q["hashes"])
        s.aad_aa1, s.aad_aa2, s.aad_dist, s.aad_qi = q["aa1"].ctypes.data_as(_lib.u8p), q["aa2"].ctypes.data_as(_lib.u8p), q["dist"].ctypes.data_as(_lib.f32p), q["qi"].ctypes.data_as(_lib.u32p)
        s.n_aad, s.ca_distance_cutoff, s.use_aa_prefilter = len(q["dist"]), q["window"], q["prefilter"]
    cand = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint32) for c in cands] + [np.zeros(0, np.uint32)]), np.uint32)
    cand_off = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.uint64)
    res_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    blk, lay, sc, msg = _lib.u32p(), (C.c_uint64 * 16)(), (C.c_uint64 * 5)(), C.c_char_p()
    rc = _lib.load().fdgpu_debug_match_tables(len(queries), qs, cand.ctypes.data_as(_lib.u32p) if len(cand) else None, cand_off.ctypes.data_as(_lib.u64p),
                                              res_off.ctypes.data_as(_lib.u64p), len(lens), hash_type, int(dev_items), int(pooled), C.byref(blk), lay, sc, C.byref(msg))
    out = dict(rc=rc, msg=msg.value.decode() if msg.value else None)
    if rc == 0:
        L = out["L"] = dict(zip(LAYOUT, [int(x) for x in lay]))
        out["blk"] = np.ctypeslib.as_array(blk, shape=(L["words"],)).copy()
        _libc.free(C.cast(blk, C.c_void_p))
        out.update(n_wi=int(sc[0]), j_span=int(sc[1]), want_iv=int(sc[2]), qset_slots=int(sc[3]), qset_max=int(sc[4]), nq=len(queries), n_cand=len(cand))
    return out


def section(b, name, n, dtype=np.uint32):
    return b["blk"][b["L"][name]:b["L"][name] + n].view(dtype)


def qtab(b, t):
    w = section(b, "qtab", 10 * b["nq"])[10 * t:10 * t + 10]
    return dict(zip(QTAB, [int(x) for x in w]), ca_window=w[7:8].view(np.float32)[0])


# ------------------------------------------------------------------------------------------------------------ start tables and group order
def grouped_witness(q):
    """stable sort of the entries with both residue types below 32 by aa1 * 32 + aa2 -> (start[1025], dist, qi)"""
    keep = (q["aa1"] < 32) & (q["aa2"] < 32)
    key = q["aa1"][keep].astype(np.int64) * 32 + q["aa2"][keep]
    order = np.argsort(key, kind="stable")
    return np.searchsorted(key[order], np.arange(1025), "left").astype(np.uint32), q["dist"][keep][order], q["qi"][keep][order]


def observed(n, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    types = np.array([0, 3, 19, 31, 32, 255], np.uint8)          # 16 groups survive, several entries each; types >= 32 are dropped
    return types[rng.integers(0, 6, n)], types[rng.integers(0, 6, n)], rng.uniform(3.0, 20.0, n).astype(np.float32), rng.integers(0, 50, n).astype(np.uint32)


def start_query(n, last=None):
    a1, a2, d, qi = (x[:n].copy() for x in observed(1025))          # every size is a prefix of the same list: 257 = the 256 case + one entry
    if last is not None:
        a1[-1], a2[-1] = last
    return query([1 << 25], a1, a2, d, qi)


@pytest.mark.parametrize("n_aad", (0, 1, 255, 256, 257, 1025))
def test_start_table_and_group_order(n_aad):
    q = start_query(n_aad)
    front = query([5], [1, 0, 0], [1, 0, 0], [4.0, 5.0, 6.0])          # a query in front: aad_off and the start table's place are the second query's own
    b = build([front, q], [[0], [0]], [10], dev_items=1)
    assert b["rc"] == 0 and not b["want_iv"]
    start, dist, qi = grouped_witness(q)
    Q = qtab(b, 1)
    assert Q["n_aad"] == len(dist) and Q["aad_off"] == 3 and qtab(b, 0)["n_aad"] == 3
    assert np.array_equal(section(b, "start", 2050)[1025:], start) and np.array_equal(section(b, "start", 1025), grouped_witness(front)[0])
    assert section(b, "dist", 3 + len(dist), np.float32)[3:].tobytes() == dist.tobytes() and np.array_equal(section(b, "qi", 3 + len(qi)), [1, 2, 0] + qi.tolist())
    if n_aad >= 255:
        assert set(q["aa1"].tolist()) >= {31, 32, 255} and np.diff(start).max() > 1 and len(dist) < n_aad


def test_both_construction_paths_agree():
    """257 entries whose last is dropped (counting sort) == the first 256 (sorted keys); a kept 257th lands at the end of its group"""
    b256, b257 = (build([start_query(256)], [[0]], [10], dev_items=1), build([start_query(257, last=(255, 0))], [[0]], [10], dev_items=1))
    n = qtab(b256, 0)["n_aad"]
    assert qtab(b257, 0)["n_aad"] == n
    for name, cnt in (("start", 1025), ("dist", n), ("qi", n)):
        assert np.array_equal(section(b256, name, cnt), section(b257, name, cnt)), name
    kept = start_query(257, last=(3, 19))
    b = build([kept], [[0]], [10], dev_items=1)
    start, dist, qi = grouped_witness(kept)
    assert np.array_equal(section(b, "start", 1025), start) and np.array_equal(section(b, "qi", n + 1), qi)
    assert int(section(b, "qi", n + 1)[start[3 * 32 + 19 + 1] - 1]) == int(kept["qi"][-1])


# ------------------------------------------------------------------------------------------------------------ interval tables
WINDOWS = (1.0, 3.0, 1e-6, 0.0, -1.0, float("nan"))
G_OVERLAP, G_ONE_ULP, G_TWO_ULP, G_MANY, G_FILL = (0, 0), (0, 1), (0, 2), (0, 3), (1, 1)


def interval_query(window):
    rng = np.random.Generator(np.random.PCG64(11))
    below7 = np.nextafter(f32(7.0), f32(0.0))
    groups = {G_OVERLAP: [5.0, 5.5, 9.0], G_ONE_ULP: [5.0, below7], G_TWO_ULP: [5.0, 7.0], G_MANY: [4.0 + 3.0 * k for k in range(256)],
              G_FILL: rng.uniform(3.0, 20.0, 1100)}
    a1 = np.concatenate([np.full(len(v), g[0]) for g, v in groups.items()])
    a2 = np.concatenate([np.full(len(v), g[1]) for g, v in groups.items()])
    d = np.concatenate([np.asarray(v, np.float32) for v in groups.values()])
    p = rng.permutation(len(d))          # groups interleaved in the observed list
    return query([1 << 25], a1[p], a2[p], d[p], window=window)


def passes(d, x, w):
    with np.errstate(invalid="ignore"):
        return (np.abs((d[:, None] - x[None, :]).astype(np.float32)) < f32(w)).any(axis=1)


def neighbours(v):
    v = np.asarray(v, np.float32)
    return np.concatenate([v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))])


@pytest.fixture(scope="module")
def iv_block():
    qs = [interval_query(w) for w in WINDOWS]
    return qs, build(qs, [[0]] * len(qs), [10], dev_items=0)


@pytest.mark.parametrize("t", range(len(WINDOWS)))
def test_intervals_equal_the_window_test(iv_block, t):
    qs, b = iv_block
    assert b["rc"] == 0 and b["want_iv"] and qtab(b, t)["n_aad"] > 1024
    w = f32(WINDOWS[t])
    start, dist, _ = grouped_witness(qs[t])
    nq = len(qs)
    iv_start = section(b, "iv_start", 1025 * nq)[1025 * t:1025 * (t + 1)].astype(np.int64)
    n_iv = int(section(b, "iv_start", 1025 * nq)[1025 * nq - 1])
    iv = section(b, "iv", 2 * n_iv, np.float32).reshape(-1, 2)
    grp = section(b, "iv_grp", 1024 * nq)[1024 * t:1024 * (t + 1)]
    assert np.all(np.diff(iv_start) >= 0)
    assert np.array_equal(grp, (np.minimum(iv_start[:-1] - iv_start[0], 0xffffff) << 8) | np.minimum(np.diff(iv_start), 255))
    for g in range(1024):
        x, I = dist[start[g]:start[g + 1]], iv[iv_start[g]:iv_start[g + 1]]
        if not (w > 0):          # 0, negative, NaN: nothing passes
            assert len(I) == 0
        if len(x) == 0:
            assert len(I) == 0
            continue
        assert np.all(I[:, 0] <= I[:, 1]) and np.all(np.nextafter(I[:-1, 1], f32(np.inf)) < I[1:, 0])          # ascending, with a float between neighbours
        d = neighbours(np.concatenate([I.ravel(), x + w, x - w]))
        inside = ((d[:, None] >= I[None, :, 0]) & (d[:, None] <= I[None, :, 1])).any(axis=1)
        assert np.array_equal(inside, passes(d, x, w)), (t, g)


def test_interval_merging_at_one_and_two_ulps(iv_block):
    qs, b = iv_block
    iv_start = section(b, "iv_start", 1025)          # query 0: window 1.0
    count = lambda g: int(iv_start[g[0] * 32 + g[1] + 1] - iv_start[g[0] * 32 + g[1]])
    six, below6, above6, below7 = f32(6.0), np.nextafter(f32(6.0), f32(0.0)), np.nextafter(f32(6.0), f32(9.0)), np.nextafter(f32(7.0), f32(0.0))
    # the premises, in float32: 5.0 passes up to the float below 6; the float below 7 passes from 6 on (adjacent floats: one ulp apart), 7.0 only from
    # the float above 6 (6.0 lies between: two ulps apart)
    assert passes(np.array([below6, six]), np.array([5.0], np.float32), 1.0).tolist() == [True, False]
    assert passes(np.array([below6, six]), np.array([below7]), 1.0).tolist() == [False, True]
    assert passes(np.array([six, above6]), np.array([7.0], np.float32), 1.0).tolist() == [False, True]
    assert count(G_OVERLAP) == 2 and count(G_ONE_ULP) == 1 and count(G_TWO_ULP) == 2
    assert count(G_MANY) == 256 and int(section(b, "iv_grp", 1024)[G_MANY[0] * 32 + G_MANY[1]]) & 0xff == 255          # the count saturates


def test_pooled_intervals_equal_serial():
    rng = np.random.Generator(np.random.PCG64(13))
    n = 9000
    q = query([1 << 25], rng.integers(0, 20, n), rng.integers(0, 20, n), np.round(rng.uniform(3.0, 20.0, n), 3), window=1.0)
    serial, pooled = (build([q], [[0]], [10], dev_items=0, pooled=p) for p in (0, 1))
    assert serial["want_iv"] and qtab(serial, 0)["n_aad"] >= 8192
    assert serial["L"] == pooled["L"] and serial["blk"].tobytes() == pooled["blk"].tobytes()


# ------------------------------------------------------------------------------------------------------------ work items
def items_witness(cands, lens, j_span):
    res_off = np.concatenate([[0], np.cumsum(lens)])
    out, k = [], 0
    for t, cs in enumerate(cands):
        for s in cs:
            r0, r1 = int(res_off[s]), int(res_off[s + 1])
            out += [(k, r, t, j0) for r in range(r0, r1, 64) for j0 in range(r0, r1, j_span)]
            k += 1
    return np.array(out, np.uint32).reshape(-1, 4)


def test_work_items_in_both_forms():
    lens = [130, 0, 64, 65, 300]          # a zero-length structure among them
    cands = [[0, 1, 4], [], [3, 2, 1, 0]]
    q = query([1 << 25], [0], [0], [5.0])
    host, dev = (build([q, q, q], cands, lens, dev_items=d) for d in (0, 1))
    assert host["j_span"] == dev["j_span"] == 64
    W = items_witness(cands, lens, 64)
    assert host["n_wi"] == dev["n_wi"] == len(W)
    for z, name in enumerate(("wc", "wi", "wq", "wj")):
        assert np.array_equal(section(host, name, len(W)), W[:, z]), name
    first = np.concatenate([[0], np.cumsum(np.bincount(W[:, 0], minlength=7))])
    assert np.array_equal(section(dev, "wbase", 8), first) and np.array_equal(section(dev, "cq", 7), [0, 0, 0, 2, 2, 2, 2])
    assert first[2] == first[1] and np.array_equal(section(dev, "cand", 7), [0, 1, 4, 3, 2, 1, 0])


@pytest.mark.parametrize("n_cand,n_aad,j_span", ((255, 1, 64), (256, 1, 128), (1023, 1, 128), (1024, 1, 256), (1024, 4096, 256), (1024, 4097, 128)))
def test_j_span_switches(n_cand, n_aad, j_span):
    """n_cand candidates of one 64-residue tile each; the longest observed list counts as given (dropped entries included)"""
    q = query([1 << 25], np.full(n_aad, 255), np.full(n_aad, 255), np.zeros(n_aad))
    for d in (0, 1):
        b = build([q], [[0] * n_cand], [64], dev_items=d)
        assert b["rc"] == 0 and b["j_span"] == j_span and b["n_wi"] == n_cand


def test_no_candidates_and_refusals():
    q = query([1 << 25], [0], [0], [5.0])
    for d in (0, 1):
        b = build([q], [[]], [64], dev_items=d)
        assert b["rc"] == 0 and b["n_wi"] == 0 and b["j_span"] == 0
        bad = build([q], [[0, 2]], [64, 64], dev_items=d)
        assert bad["rc"] == EINVAL and bad["msg"] == "match_pairs: candidate id outside the batch"
    big = build([q], [[0] * 256], [65535], dev_items=1)          # 256 x 1,024 tiles x 256 spans = 2^26 items; only the lengths are read
    assert big["rc"] == ERANGE and big["msg"] == "match_pairs: more than 2^26 work items in one call; split the candidates"
    assert build([q], [[0] * 255], [65535], dev_items=1)["n_wi"] == 255 << 18


# ------------------------------------------------------------------------------------------------------------ hash sets, masks, prefilter
def test_hash_set_slots_and_query_words():
    h = lambda n: (np.arange(n, dtype=np.uint32) << 8) | (7 << 25) | (9 << 20)          # default encoding: residue types at bits 25 and 20
    small, large = query(h(1024), window=2.5), query(h(1025))
    b = build([small, large, large], [[0], [0], [0]], [10], dev_items=1)
    assert b["qset_slots"] == 8192 and b["qset_max"] == 1025
    Q = [qtab(b, t) for t in range(3)]
    assert [(x["qs_off"], x["qs_mask"]) for x in Q] == [(0, 0), (0, 4095), (4096, 4095)]
    assert [(x["qh_off"], x["n_hashes"]) for x in Q] == [(0, 1024), (1024, 1025), (2049, 1025)] and np.array_equal(section(b, "hashes", 3074)[1024:2049], large["hashes"])
    assert (Q[0]["aa1_mask"], Q[0]["aa2_mask"]) == (1 << 7, 1 << 9) and Q[1]["aa2_mask"] == 1 << 9 and Q[0]["ca_window"] == f32(2.5)
    assert build([small], [[0]], [10], dev_items=1)["qset_slots"] == 0
    # the two encodings without residue types never prefilter
    assert [qtab(build([small], [[0]], [10], dev_items=1, hash_type=ht), 0)["use_prefilter"] for ht in (3, 5, 6)] == [1, 0, 0]


# ------------------------------------------------------------------------------------------------------------ layout
def test_layout_sections(iv_block):
    q = query([1 << 25, 2 << 25, 3 << 25], [0, 1, 2], [0, 1, 2], [5.0, 6.0, 7.0])
    small = [build([q, q], [[0, 1], [1]], [70, 3], dev_items=d) for d in (0, 1)]
    for b in small + [iv_block[1]]:
        L, nq, nc, nw = b["L"], b["nq"], b["n_cand"], b["n_wi"]
        na, nh = sum(qtab(b, t)["n_aad"] for t in range(nq)), sum(qtab(b, t)["n_hashes"] for t in range(nq))
        n_iv = int(section(b, "iv_start", 1025 * nq)[-1]) if b["want_iv"] else 0
        dev = b is small[1]
        size = dict(cand=nc, wc=nw, wi=nw, wq=nw, wj=nw, hashes=nh, start=1025 * nq, dist=na, qi=na, qtab=10 * nq, iv_start=1025 * nq if b["want_iv"] else 0,
                    iv=2 * n_iv, iv_grp=1024 * nq if b["want_iv"] else 0, wbase=nc + 1 if dev else 0, cq=nc if dev else 0)
        assert all(L[k] % 4 == 0 for k in LAYOUT[:-1])
        for k, nxt in zip(LAYOUT[:-1], LAYOUT[1:]):
            assert L[k] + size[k] <= L[nxt], (k, L)
