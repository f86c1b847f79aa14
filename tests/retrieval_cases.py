"""Hand-made query maps for the retrieval side (fdgpu_retrieve_batch: the pair scan of k_match.hip and the per-candidate glue of k_retrieve.hip) at the
limits and form switches of its dispatch, with a plain Python model of the whole glue (pair scan, graph, components, votes, assignment, rescue) beside
the oracle.  No GPU, nothing committed as data: every structure comes from folddisco_amd.synth.generate with a fixed seed and explicit lengths.

A query map does not have to come from make_query_map: the retrieval reads a caller-visible fd_query_map, the oracle an fdo_query_map, and both are
filled here from one set of numpy arrays (MapBuilder.arrays): hash -> (qi, qj, idf), `indices`, and the observed-distance list (aa1, aa2, dist, qi).
The target of a case is the query structure itself, so that the hash of target pair (i, j) (oracle.pair_hash) put into the map draws the directed edge
i -> j into the first candidate's match graph; a second candidate (the same structure with 0.03 A of noise) stands beside it as the ordinary slot.  Edges
are taken from pairs whose hash occurs once in the structure (Struct.uniq), so the number of found triples is the number of edges; what collisions and
same-type pairs at a similar distance add (candidate pairs mostly) is counted by the model, and test_retrieval_cases_host.py checks every claim against
the oracle's own output.

Fields of fd_query_map the retrieval reads (fd_retrieve_host.cpp: fd_rb_prepare, fd_rh_slot; fd_host_query.hip: rs_pack_tables): n, hash, qi, qj, idf, n_indices,
indices, n_aad, aad_aa1, aad_aa2, aad_dist, aad_qi.  Nothing else: is_primary is never read there, primary_hash is set to `hash` as make_query_map
does, post_len / post_seg / post_kidx stay NULL and post_index_uid / arena_bytes 0 (they belong to the scoring stage).  library_map() wraps the struct in
QueryMapResult(None, pointer): with no context the wrapper never hands the hand-made struct to fdgpu_query_map_free.

Every idf is a multiple of 2^-8 below 1/4: the f32 sum over at most 4,097 edges is exact in any order and is compared bit for bit.

Thresholds come from the sources' #defines (RS_* of k_retrieve.hip, MP_* of k_match.hip / fdgpu_internal.h); the ones that are literals in the code are
restated here: 64 graph nodes / query residues (FD_WAVE), 200 hashes (prefilter), 256 hashes held in LDS by k_rs_setup (2 * RS_S_EDGE), 256 sorted keys of
the observed-distance table, 4096 observed distances (two-pass).

Case classes (CLASSES; `claims` states as data what a case exists for, `path` which way the call goes: "device" = the device glue ran to the end,
"overflow" = it raised its flag and the call came back through the host path, "host" = the device glue was never started):
  nodes   63 / 64 / 65 graph nodes in the first candidate as a two-way chain, a one-way ring and a one-way star; at 64 the chain is one component that
          holds node 63, `tail64_nc1` leaves node 63 alone in its own component (node_count = 1); 65 nodes overflow.
  edges   F = 127 / 128 / 129 found triples (k_rs_setup hands slots above RS_S_EDGE to k_rs_slots; the noisy second candidate stays below, so the list
          holds some slots and not others) and F = 1023 / 1024 / 1025 (RS_EDGE_CAP: 1025 overflows).
  comps   two SCCs joined one way (three records); a ring alone (one); the SCC {0, 1} beside the WCC {0, 1, 2} and {1, 2} beside {0, 1, 2} (rs_less's
          two prefix branches, orders that differ from order by lowest member and by size); 64 one-way pairs' worth of singletons: 32 pairs with
          node_count = 1 give 96 components, a 64-node star 65; node_count 1, 2, 3 and 4 on the three-node graph (4: no record); a map whose
          hashes no candidate carries (no found triple).
  votes   two target residues tied for one query residue (the smaller wins); two query residues with the same best target (the second is skipped);
          the assignment stopping at the component's size; one hash on two entries (the first wins); a symmetric hash whose entry lists the query
          residues in descending order beside an asymmetric one; duplicates in `indices` (the erase-and-reinsert branch, with the erased position
          equal to and different from the first occurrence); 64 / 65 distinct query residues with a vote in one component (65 overflows); a pair voted
          more than 255 times (u8 saturation) where the saturation changes the winner — built as a host-path case (161 nodes: the device glue
          declines), not with multiple_bins; 4096 / 4097 found triples and hashes in one slot (the host glue's dense vote table and its hash ->
          entry table, fd_retrieve_host.cpp).
  rescue  largest tally 1 (none); a unique 2 (rescue); two residues tied at 2 (none); the unique largest already assigned (none); a residue of
          `indices` without any observed distance; C = 511 / 512 / 513 candidate pairs in the slot (RS_CAND_LDS) and 511 / 512 / 513 candidate pairs whose
          partner the component assigned (RS_S_FILT), each with a rescue that the last candidate pairs of the slot decide; 511 / 512 / 513 voting pairs of
          one unmatched residue in the split form's unfiltered walk (RS_S_LIST; 513 overflows there only) and 2047 / 2048 / 2049 in a slot of 129 found
          triples (RS_LIST_CAP of k_rs_slots; 2049 overflows).  The same two caps on the VOTE lists cannot be met: a component has at most two votes per
          found triple, and a slot has at most RS_S_EDGE (RS_EDGE_CAP) triples before it is handed over (declined) — 2 * 128 < 512, 2 * 1024 = 2048.
  sizes   63 / 64 / 65 entries in `indices` (65: host glue from the start); 200 / 201, 256 / 257, 1024 / 1025 and 2048 / 2049 distinct hashes; n_aad
          256 / 257, 1024 / 1025 and 4096 / 4097 (two-pass).
  window  an observed distance x with |d - x| one ulp inside, exactly on and one ulp outside ca_distance_cutoff on both sides of d, for 1.0, 1.5
          and 3.0; cutoff 0.0 and NaN; residue types 20, 31, 32, 33 and 255; beyond 1,024 entries overlapping and abutting windows of one type pair.
  long    targets of 4096 and 4097 residues with a six-edge map."""
import collections
import ctypes as C
import functools
import os
import re

import numpy as np

import oracle

SEED = 20261018
CLASSES = ("nodes", "edges", "comps", "votes", "rescue", "sizes", "window", "long")
WAVE, PREFILTER, SETUP_HASH_LDS, AAD_SORTED, TWO_PASS_AAD = 64, 200, 256, 256, 4096
HOST_DENSE = 4096          # fd_retrieve_host.cpp: found triples of a slot above which its votes go through a dense table, hashes of a query above which
                           # they are looked up in a table


def _define(fname, name):
    import folddisco_amd
    text = open(os.path.join(os.path.dirname(folddisco_amd.__file__), "csrc", fname)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


RS_EDGE_CAP, RS_LIST_CAP, RS_CAND_LDS = (_define("k_retrieve.hip", n) for n in ("RS_EDGE_CAP", "RS_LIST_CAP", "RS_CAND_LDS"))
RS_S_EDGE, RS_S_LIST, RS_S_FILT = (_define("k_retrieve.hip", n) for n in ("RS_S_EDGE", "RS_S_LIST", "RS_S_FILT"))
MP_AAD_LDS, MP_SCAN_BLOCKS, MP_QH_LDS = _define("k_match.hip", "MP_AAD_LDS"), _define("k_match.hip", "MP_SCAN_BLOCKS"), _define("fdgpu_internal.h", "MP_QH_LDS")
assert SETUP_HASH_LDS == 2 * RS_S_EDGE

MAP_KEYS = ("hash", "qi", "qj", "idf", "indices", "aad_aa1", "aad_aa2", "aad_dist", "aad_qi")


# ---------------------------------------------------------------------------------------------------------------- structures
class Struct:
    """one structure: the arrays both sides are fed with, the oracle's structure, the f32 CA distances as the scan computes them"""

    def __init__(self, item):
        self.item = item
        self.aa = np.ascontiguousarray(item["aa"], np.uint8)
        self.n = len(self.aa)
        self.o = oracle.structure_from_packed(item["n_xyz"], item["ca_xyz"], item["cb_xyz"], self.aa)
        self._h = {}

    @functools.cached_property
    def D(self):
        ca = np.ascontiguousarray(self.item["ca_xyz"], np.float32)
        d = [ca[:, None, k] - ca[None, :, k] for k in range(3)]
        return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])          # sqrtf(dx * dx + dy * dy + dz * dz), no contraction

    @functools.cached_property
    def valid(self):
        return (self.D <= np.float32(20.0)) & ~np.eye(self.n, dtype=bool)

    def h(self, i, j):
        k = (int(i), int(j))
        if k not in self._h:
            r = oracle.pair_hash(self.o, k[0], k[1])
            self._h[k] = None if r is None else r[0]
        return self._h[k]

    @functools.cached_property
    def hash_count(self):
        """how many ordered pairs of the structure carry each hash (small structures only)"""
        ii, jj = np.nonzero(self.valid)
        return collections.Counter(self.h(i, j) for i, j in zip(ii.tolist(), jj.tolist()))

    def uniq(self, i, j):
        return i != j and bool(self.valid[i, j]) and self.h(i, j) is not None and self.hash_count[self.h(i, j)] == 1


@functools.lru_cache(maxsize=None)
def base(length, seed=SEED):
    from folddisco_amd import synth
    ps = synth.to_packed(synth.generate(1, seed=seed, lengths=np.array([length])))
    return Struct(dict(n_xyz=ps.n_xyz, ca_xyz=ps.ca_xyz, cb_xyz=ps.cb_xyz, aa=ps.aa, cb_ok=None))


@functools.lru_cache(maxsize=None)
def noisy(length, seed=SEED):
    """the ordinary candidate beside the limit candidate: the same structure with 0.03 A of noise, at PDB precision"""
    t = base(length, seed)
    rng = np.random.Generator(np.random.PCG64(seed + length))
    it = {k: (np.round((t.item[k] + rng.normal(0.0, 0.03, t.item[k].shape)) * 1000.0) / 1000.0).astype(np.float32) for k in ("n_xyz", "ca_xyz", "cb_xyz")}
    return Struct(dict(it, aa=t.aa, cb_ok=None))


# ---------------------------------------------------------------------------------------------------------------- the two maps from one set of arrays
def default_idf(i, j):
    return np.float32(((7 * i + 13 * j) % 61 + 1) / 256.0)


class MapBuilder:
    def __init__(self, T):
        self.T, self.ent, self.aad = T, [], []

    def edge(self, i, j, qi=None, qj=None, idf=None, obs=True):
        """target pair (i, j)'s hash -> (qi, qj, idf) (identity by default) and the pair's own observed distance for query residue qi"""
        h = self.T.h(i, j)
        assert h is not None, (i, j)
        qi, qj = i if qi is None else qi, j if qj is None else qj
        self.ent.append((h, qi, qj, default_idf(i, j) if idf is None else np.float32(idf)))
        if obs:
            self.obs(i, j, qi)
        return self

    def obs(self, i, j, q, dist=None):
        self.aad.append((int(self.T.aa[i]), int(self.T.aa[j]), np.float32(self.T.D[i, j] if dist is None else dist), q))
        return self

    def raw_obs(self, a1, a2, dist, q):
        self.aad.append((a1, a2, np.float32(dist), q))
        return self

    def raw_hash(self, h, qi, qj, idf=1.0 / 256.0):
        self.ent.append((int(h), qi, qj, np.float32(idf)))
        return self

    def arrays(self, indices):
        e, a = self.ent, self.aad
        out = dict(hash=np.array([x[0] for x in e], np.uint32), qi=np.array([x[1] for x in e], np.uint32), qj=np.array([x[2] for x in e], np.uint32),
                   idf=np.array([x[3] for x in e], np.float32), indices=np.array(indices, np.uint32),
                   aad_aa1=np.array([x[0] for x in a], np.uint8), aad_aa2=np.array([x[1] for x in a], np.uint8),
                   aad_dist=np.array([x[2] for x in a], np.float32), aad_qi=np.array([x[3] for x in a], np.uint32))
        assert np.all(out["idf"] * 256.0 == np.round(out["idf"] * 256.0)) and float(out["idf"].astype(np.float64).sum()) < 65536.0
        return out


class HandMap:
    """what oracle.retrieve(target, query, m) accepts: .ptr -> an fdo_query_map over arrays this object keeps alive (never freed by the oracle)"""

    def __init__(self, a):
        k = self._keep = dict(hash=np.ascontiguousarray(a["hash"], np.uint32), qi=np.ascontiguousarray(a["qi"], np.uint64), qj=np.ascontiguousarray(a["qj"], np.uint64),
                              is_primary=np.ones(len(a["hash"]), np.uint8), idf=np.ascontiguousarray(a["idf"], np.float32),
                              indices=np.ascontiguousarray(a["indices"], np.uint64), aad_aa1=np.ascontiguousarray(a["aad_aa1"], np.uint8),
                              aad_aa2=np.ascontiguousarray(a["aad_aa2"], np.uint8), aad_dist=np.ascontiguousarray(a["aad_dist"], np.float32),
                              aad_qi=np.ascontiguousarray(a["aad_qi"], np.uint64))
        p = lambda name, t: k[name].ctypes.data_as(t)
        self.struct = oracle.QueryMap(len(k["hash"]), p("hash", oracle.u32p), p("qi", oracle.u64p), p("qj", oracle.u64p), p("is_primary", oracle.u8p), p("idf", oracle.f32p),
                                      len(k["indices"]), p("indices", oracle.u64p), len(k["aad_dist"]), p("aad_aa1", oracle.u8p), p("aad_aa2", oracle.u8p),
                                      p("aad_dist", oracle.f32p), p("aad_qi", oracle.u64p))
        self.ptr = C.pointer(self.struct)


def oracle_map(a):
    return HandMap(a)


def library_map(a):
    """-> a QueryMapResult that query.retrieve_batch accepts (.handle, .indices) and the library never frees; the arrays live as long as the object"""
    from folddisco_amd import _lib
    from folddisco_amd.query import QueryMapResult
    k = dict(hash=np.ascontiguousarray(a["hash"], np.uint32), qi=np.ascontiguousarray(a["qi"], np.uint32), qj=np.ascontiguousarray(a["qj"], np.uint32),
             is_primary=np.ones(len(a["hash"]), np.uint8), idf=np.ascontiguousarray(a["idf"], np.float32), indices=np.ascontiguousarray(a["indices"], np.uint32),
             aad_aa1=np.ascontiguousarray(a["aad_aa1"], np.uint8), aad_aa2=np.ascontiguousarray(a["aad_aa2"], np.uint8),
             aad_dist=np.ascontiguousarray(a["aad_dist"], np.float32), aad_qi=np.ascontiguousarray(a["aad_qi"], np.uint32))
    p = lambda name, t: k[name].ctypes.data_as(t)
    s = _lib.QueryMap()
    s.n, s.hash, s.qi, s.qj, s.is_primary, s.idf = len(k["hash"]), p("hash", _lib.u32p), p("qi", _lib.u32p), p("qj", _lib.u32p), p("is_primary", _lib.u8p), p("idf", _lib.f32p)
    s.n_indices, s.indices = len(k["indices"]), p("indices", _lib.u32p)
    s.n_aad, s.aad_aa1, s.aad_aa2, s.aad_dist, s.aad_qi = len(k["aad_dist"]), p("aad_aa1", _lib.u8p), p("aad_aa2", _lib.u8p), p("aad_dist", _lib.f32p), p("aad_qi", _lib.u32p)
    s.primary_hash = p("hash", _lib.u32p)          # post_len / post_seg / post_kidx NULL, post_index_uid / arena_bytes 0: the struct starts zeroed
    qm = QueryMapResult(None, C.pointer(s))
    qm._keep = (k, s)
    return qm


def match_query(a):
    """the dict match.match_pairs builds its fd_match_query from (it sorts and dedups the hashes itself)"""
    return {k: a[k] for k in ("hash", "aad_aa1", "aad_aa2", "aad_dist", "aad_qi")}


# ---------------------------------------------------------------------------------------------------------------- the model
def model_scan(T, a, cutoff):
    """retrieve_with_prefilter restated with numpy: -> (found [n, 3] = i, j, hash; cand [m, 3] = qi, i, j), both in (i, j, emission) order"""
    hashes = set(int(h) for h in a["hash"])
    if not hashes or T.n == 0:
        return np.zeros((0, 3), np.uint64), np.zeros((0, 3), np.uint64)
    ok = T.valid.copy()
    if len(a["hash"]) <= PREFILTER:          # residue types of the hashes' two fields; both sets must be non-empty in the target
        s1 = np.isin(T.aa, [(h >> 25) & 31 for h in hashes])
        s2 = np.isin(T.aa, [(h >> 20) & 31 for h in hashes])
        if s1.any() and s2.any():
            ok &= s1[:, None] & s2[None, :]
    cut = np.float32(cutoff)
    by_type = {}
    rows = []
    for e in range(len(a["aad_dist"])):
        t = (int(a["aad_aa1"][e]), int(a["aad_aa2"][e]))
        if t not in by_type:
            ii, jj = np.nonzero(ok & (T.aa[:, None] == t[0]) & (T.aa[None, :] == t[1]))
            by_type[t] = (ii, jj, T.D[ii, jj])
        ii, jj, dd = by_type[t]
        with np.errstate(invalid="ignore"):
            m = np.abs(dd - a["aad_dist"][e]) < cut
        if m.any():
            rows.append(np.stack([ii[m], jj[m], np.full(int(m.sum()), e)], axis=1))
    if not rows:
        return np.zeros((0, 3), np.uint64), np.zeros((0, 3), np.uint64)
    r = np.concatenate(rows)
    r = r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]
    cand = np.stack([a["aad_qi"][r[:, 2]].astype(np.uint64), r[:, 0].astype(np.uint64), r[:, 1].astype(np.uint64)], axis=1)
    pairs = np.unique(r[:, :2], axis=0)
    found = [(i, j, T.h(i, j)) for i, j in pairs.tolist() if T.h(i, j) in hashes]
    return np.array(found, np.uint64).reshape(-1, 3), cand


def component_order(node_sets):
    """graph.rs:43-45 in plain Python: ascending node lists, the list of lists sorted, duplicates dropped"""
    lists = sorted(sorted(s) for s in node_sets)
    return [c for k, c in enumerate(lists) if k == 0 or c != lists[k - 1]]


def model_glue(found, cand, a, node_count):
    """graph -> components -> votes -> greedy assignment -> residue lists with the rescue, per component in the reference's order.
    -> dict(nodes = residues in first-appearance order, comps = node lists, records = [dict(from_hash, processed, idf, flags ...)])"""
    sym = lambda h: bool(oracle.lib().fdo_hash_is_symmetric(int(h)))
    nodes, idx, es = [], {}, []
    for i, j, h in found.tolist():
        for r in (i, j):
            if r not in idx:
                idx[r] = len(nodes)
                nodes.append(r)
        es.append((idx[i], idx[j], h))
    n = len(nodes)
    A = np.zeros((n, n), bool)
    for s, t, _ in es:
        A[s, t] = True

    def closure(M):
        R = M | np.eye(n, dtype=bool)
        while True:
            R2 = R | ((R.astype(np.uint8) @ R.astype(np.uint8)) > 0)
            if np.array_equal(R2, R):
                return R
            R = R2
    R, W = closure(A), closure(A | A.T)
    sets = [np.flatnonzero(R[v] & R[:, v]).tolist() for v in range(n)] + [np.flatnonzero(W[v]).tolist() for v in range(n)]
    comps = component_order([s for s in sets if len(s) >= node_count and len(s) > 0])
    first = {}
    for k, h in enumerate(a["hash"].tolist()):
        first.setdefault(h, k)
    q_size = int(max(a["qi"].max(initial=0), a["qj"].max(initial=0))) + 1 if len(a["hash"]) else 1
    records = []
    for comp in comps:
        inc = set(comp)
        counts, raw, order, idf = {}, {}, [], np.float32(0.0)
        for s, t, h in es:
            if s not in inc or t not in inc or h not in first:
                continue
            k = first[h]
            idf = np.float32(idf + a["idf"][k])
            qi, qj, ri, rj = int(a["qi"][k]), int(a["qj"][k]), nodes[s], nodes[t]
            prs = ((min(qi, qj), min(ri, rj)), (max(qi, qj), max(ri, rj))) if sym(h) else ((qi, ri), (qj, rj))
            for p in prs:
                if p not in counts:
                    order.append(p)
                counts[p] = min(counts.get(p, 0) + 1, 255)
                raw[p] = raw.get(p, 0) + 1
        best, tie = {}, False
        for q, r in order:
            c = counts[(q, r)]
            if q not in best or c > best[q][0] or (c == best[q][0] and r < best[q][1]):
                best[q] = (c, r)
        for q in best:
            tie = tie or sum(1 for (q2, r2) in order if q2 == q and counts[(q2, r2)] == best[q][0]) > 1
        # would the winner of some query residue be another without the u8 saturation?
        sat_winner = any(min((-raw[(q2, r2)], r2) for (q2, r2) in order if q2 == q)[1] != best[q][1] for q in best)
        q_idx, r_idx, skipped, stopped = [], [], False, False
        for c, q in sorted(((-best[q][0], q) for q in best)):
            if len(q_idx) == len(comp):
                stopped = True
                break
            if best[q][1] in r_idx:
                skipped = True
                continue
            q_idx.append(q)
            r_idx.append(best[q][1])
        NQ = len(a["indices"])
        fh, pr, qs, rs = [-1] * NQ, [-1] * NQ, [], []
        quirk, quirk_other, rescued, tallies, tally_len = False, False, [], {}, 0
        for pos in range(NQ):
            qi = int(a["indices"][pos])
            if qi in q_idx:
                mapped = r_idx[q_idx.index(qi)]
                fh[pos] = mapped
                if mapped not in rs:
                    pr[pos] = mapped
                else:
                    pp = rs.index(mapped)
                    quirk = True
                    quirk_other = quirk_other or pr[pp] != mapped
                    pr[pp] = -1
                    pr[pos] = mapped
                    del qs[pp], rs[pp]
                qs.append(qi)
                rs.append(mapped)
            else:
                tally = collections.OrderedDict()
                for cq, ci, cj in cand.tolist():
                    if cq == qi and cj in r_idx:
                        tally[ci] = tally.get(ci, 0) + 1
                tally_len = max(tally_len, sum(tally.values()))
                if tally:
                    mx = max(tally.values())
                    arg = [k for k, v in tally.items() if v == mx]
                    tallies[pos] = (mx, len(arg), arg[-1] in rs)
                    if len(arg) == 1 and mx >= 2 and arg[0] not in rs:
                        pr[pos] = arg[0]
                        qs.append(qi)
                        rs.append(arg[0])
                        rescued.append(pos)
        records.append(dict(from_hash=fh, processed=pr, idf=idf, same=fh == pr, n_assigned=len(q_idx), assigned=list(zip(q_idx, r_idx)), votes=len(order),
                            tie=tie, skipped=skipped, stopped=stopped, quirk=quirk, quirk_other=quirk_other, rescued=rescued, tallies=tallies,
                            filt=int(sum(1 for _, _, cj in cand.tolist() if cj in r_idx)), max_vote=max(counts.values(), default=0),
                            q_residues=len(best), tally_len=tally_len, sat_winner=sat_winner))
    return dict(nodes=nodes, comps=comps, records=records, q_size=q_size)


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, cls, T, arrays, claims, node_count=2, cutoff=1.0, path="device", targets=None, split_only=False):
        self.split_only = split_only          # the overflow is one of the split form's own limits: under FDGPU_RS_SPLIT=0 the device glue finishes
        self.name, self.cls, self.query, self.arrays, self.claims, self.node_count, self.ca_distance_cutoff, self.path = name, cls, T, arrays, claims, node_count, cutoff, path
        self.targets = targets if targets is not None else [T, noisy(T.n)]

    def __repr__(self):
        return "Case(%s/%s)" % (self.cls, self.name)


def _path(T, n, two_way=True, close=False, top=None):
    """n residues r[0], r[1], ... with every r[k] -> r[k + 1] (and back, if two_way) a pair whose hash is unique in T; close: r[n - 1] -> r[0] too;
    top: residues below `top` only"""
    top = T.n if top is None else top
    okp = (lambda u, v: T.uniq(u, v) and T.uniq(v, u)) if two_way else T.uniq
    for start in range(top):
        path, seen = [start], {start}
        while len(path) < n:
            nxt = next((v for v in range(top) if v not in seen and okp(path[-1], v)), None)
            if nxt is None:
                break
            path.append(nxt)
            seen.add(nxt)
        if len(path) == n and (not close or okp(path[-1], path[0])):
            return path
    raise AssertionError("no path of %d residues" % n)


def _fill_indices(T, want, n):
    """`want` first, then the lowest residues not in it, n entries in all"""
    out = list(want)[:n]
    out += [r for r in range(T.n) if r not in set(out)][: n - len(out)]
    assert len(out) == n
    return out


def _nodes_cases():
    T = base(70)
    out = []
    for n in (63, 64, 65):
        p = _path(T, n)
        b = MapBuilder(T)
        for u, v in zip(p, p[1:]):
            b.edge(u, v).edge(v, u)
        out.append(Case("chain%d" % n, "nodes", T, b.arrays(_fill_indices(T, sorted(p), 64)), dict(F=2 * (n - 1), nodes=n, comps=1, comp_sizes=[n], last_node_in=[n]),
                        path="device" if n <= WAVE else "overflow"))
        p = _path(T, n, two_way=False, close=True)
        b = MapBuilder(T)
        for u, v in zip(p, p[1:] + p[:1]):
            b.edge(u, v)
        out.append(Case("ring%d" % n, "nodes", T, b.arrays(_fill_indices(T, sorted(p), 64)), dict(F=n, nodes=n, comps=1, comp_sizes=[n]), path="device" if n <= WAVE else "overflow"))
        c = max(range(T.n), key=lambda r: sum(T.uniq(r, v) for v in range(T.n)))
        leaves = [v for v in range(T.n) if T.uniq(c, v)][: n - 1]
        assert len(leaves) == n - 1
        b = MapBuilder(T)
        for v in leaves:
            b.edge(c, v)
        out.append(Case("star%d" % n, "nodes", T, b.arrays(_fill_indices(T, sorted([c] + leaves), 64)), dict(F=n - 1, nodes=n, comps=1, comp_sizes=[n]),
                        path="device" if n <= WAVE else "overflow"))
    # node 63 alone in its own component: a two-way chain of 63 residues below residue y = its largest, and y -> z with z above every residue of the chain
    # (z appears last in the scan, row y's last pair); node_count = 1: the chain, {z}, and the weak component of all 64
    z = None
    for top in range(T.n - 2, 62, -1):
        try:
            p = _path(T, 63, top=top)
        except AssertionError:
            continue
        y = max(p)
        z = next((v for v in range(y + 1, T.n) if T.uniq(y, v)), None)
        if z is not None:
            break
    assert z is not None
    b = MapBuilder(T)
    for u, v in zip(p, p[1:]):
        b.edge(u, v).edge(v, u)
    b.edge(y, z)
    out.append(Case("tail64_nc1", "nodes", T, b.arrays(_fill_indices(T, sorted(p + [z]), 64)), dict(F=2 * 62 + 1, nodes=64, comps=3, comp_sizes=[63, 64, 1], last_node_in=[64, 1]),
                    node_count=1))
    return out


def _central(T, k):
    ca = T.item["ca_xyz"]
    return sorted(np.argsort(np.linalg.norm(ca - ca.mean(axis=0), axis=1), kind="stable")[:k].tolist())


def _edges_cases():
    T = base(120)
    out = []
    for F, k in ((127, 20), (128, 20), (129, 20), (1023, 45), (1024, 45), (1025, 45)):
        res = _central(T, k)
        pairs = [(i, j) for i in res for j in res if T.uniq(i, j)]
        rng = np.random.Generator(np.random.PCG64(SEED + k))
        pairs = [pairs[x] for x in rng.permutation(len(pairs))][:F]
        assert len(pairs) == F
        b = MapBuilder(T)
        for i, j in pairs:
            b.edge(i, j)
        out.append(Case("F%d" % F, "edges", T, b.arrays(_fill_indices(T, res, min(k + 4, 64))), dict(F=F, max_nodes=k, hashes=F),
                        path="device" if F <= RS_EDGE_CAP else "overflow"))
    return out


def _small(T, k, lo=0):
    """k residues r[0] < r[1] < ... from `lo` upwards whose ordered pairs all carry hashes unique in T"""
    out = []
    for r in range(lo, T.n):
        if all(T.uniq(r, s) and T.uniq(s, r) for s in out):
            out.append(r)
            if len(out) == k:
                return out
    raise AssertionError("no clique of %d" % k)


def _comps_cases():
    T = base(120)
    r = _small(T, 4)
    out = []
    g = lambda edges: [(r[u], r[v]) for u, v in edges]

    def case(name, edges, claims, node_count=2, idx=None):
        b = MapBuilder(T)
        for i, j in edges:
            b.edge(i, j)
        return Case(name, "comps", T, b.arrays(sorted({x for e in edges for x in e}) if idx is None else idx), claims, node_count=node_count)
    out.append(case("two_scc_one_way", g([(0, 1), (1, 0), (2, 3), (3, 2), (1, 2)]), dict(F=5, nodes=4, components=[[0, 1], [0, 1, 2, 3], [2, 3]])))
    out.append(case("ring_alone", g([(0, 1), (1, 2), (2, 0)]), dict(F=3, nodes=3, components=[[0, 1, 2]])))
    out.append(case("prefix_scc_first", g([(0, 1), (1, 0), (1, 2)]), dict(F=3, nodes=3, components=[[0, 1], [0, 1, 2]])))
    out.append(case("prefix_wcc_first", g([(0, 1), (1, 2), (2, 1)]), dict(F=3, nodes=3, components=[[0, 1, 2], [1, 2]])))
    for nc, comps in ((1, [[0, 1], [0, 1, 2], [2]]), (2, [[0, 1], [0, 1, 2]]), (3, [[0, 1, 2]]), (4, [])):
        out.append(case("node_count%d" % nc, g([(0, 1), (1, 0), (1, 2)]), dict(F=3, nodes=3, components=comps), node_count=nc))
    # a map none of whose hashes the candidates carry (observed distances that do match): candidate pairs, no found triple, no record
    b = MapBuilder(T).obs(r[0], r[1], r[0]).obs(r[1], r[0], r[1])
    for k, h in enumerate(_filler_hashes(T, 3)):
        b.raw_hash(h, r[k % 2], r[(k + 1) % 2])
    out.append(Case("no_hash_found", "comps", T, b.arrays(r[:2]), dict(F=0, components=[])))
    # 32 one-way pairs r[2k] -> r[2k + 1] over 64 ascending residues: node v = the v-th residue; node_count = 1: 64 singletons and 32 pairs = 96 components
    T7 = base(70)
    used, pairs = set(), []
    for u in range(T7.n):
        if u in used:
            continue
        v = next((v for v in range(u + 1, T7.n) if v not in used and T7.uniq(u, v)), None)
        if v is not None and len(pairs) < 32:
            pairs.append((u, v))
            used |= {u, v}
    assert len(pairs) == 32
    b = MapBuilder(T7)
    for u, v in pairs:
        b.edge(u, v)
    out.append(Case("pairs32_nc1", "comps", T7, b.arrays(sorted(used)), dict(F=32, nodes=64, n_components=96), node_count=1))
    c = max(range(T7.n), key=lambda x: sum(T7.uniq(x, v) for v in range(T7.n)))
    leaves = [v for v in range(T7.n) if T7.uniq(c, v)][:63]
    b = MapBuilder(T7)
    for v in leaves:
        b.edge(c, v)
    out.append(Case("star64_nc1", "comps", T7, b.arrays(sorted([c] + leaves)), dict(F=63, nodes=64, n_components=65), node_count=1))
    return out


def _votes_cases():
    T = base(120)
    r = _small(T, 6, lo=10)
    a, bq, c, d, e, f = r
    out = []

    def case(name, b, idx, claims):
        return Case(name, "votes", T, b.arrays(idx), claims)
    # a -> b as (c, b) and c -> b as (c, b): query residue c is voted a and c once each -> a (the smaller); b twice
    b = MapBuilder(T).edge(a, bq, qi=c, qj=bq).edge(c, bq, qi=c, qj=bq)
    out.append(case("tie_smaller_wins", b, [a, bq, c], dict(F=2, nodes=3, tie=True, mapping=[{c: a, bq: bq}])))
    # a -> b as (z, b) with z < a and a -> c as (a, c): a is the best target of query residues z and a -> z takes it, a is skipped
    z = a - 1
    b = MapBuilder(T).edge(a, bq, qi=z, qj=bq).edge(a, c)
    out.append(case("same_best_target", b, [z, a, bq, c], dict(F=2, nodes=3, skipped=True, mapping=[{z: a, bq: bq, c: c}])))
    # a <-> b as (a, b) and (c, d): four query residues with a vote, two nodes -> the loop ends at two assignments
    b = MapBuilder(T).edge(a, bq).edge(bq, a, qi=c, qj=d)
    out.append(case("stop_at_size", b, [a, bq, c, d], dict(F=2, nodes=2, stopped=True, mapping=[{a: a, bq: bq}])))
    # the hash of a -> b on two entries: (a, b) first, then (e, f) -> e and f stay without a target
    b = MapBuilder(T).edge(a, bq).edge(bq, c)
    b.raw_hash(T.h(a, bq), e, f, 3.0 / 256.0)
    out.append(case("first_entry_wins", b, [a, bq, c, e, f], dict(F=2, nodes=3, hashes=2, entries=3, mapping=[{a: a, bq: bq, c: c}])))
    # a symmetric hash with its entry's query residues in descending order beside an asymmetric edge
    sp = next(((i, j) for i in range(T.n) for j in range(i + 1, T.n) if T.valid[i, j] and T.h(i, j) is not None and oracle.lib().fdo_hash_is_symmetric(T.h(i, j))
               and T.hash_count[T.h(i, j)] <= 2 and T.uniq(j, next(x for x in r if x not in (i, j)))), None)
    assert sp is not None
    i, j = sp
    x = next(x for x in r if x not in (i, j))
    b = MapBuilder(T).edge(i, j, qi=j, qj=i).edge(j, x)
    out.append(case("symmetric_beside_asymmetric", b, [i, j, x], dict(nodes=3, symmetric=1, mapping=[{i: i, j: j}, {i: i, j: j, x: x}])))
    # duplicates in `indices`
    for name, idx, cl in (("dup_first", [a, bq, a], dict(quirk=True, quirk_other=False)), ("dup_behind_gap", [e, a, bq, a], dict(quirk=True, quirk_other=True)),
                          ("dup_adjacent", [bq, c, a, a], dict(quirk=True, quirk_other=False))):
        b = MapBuilder(T).edge(a, bq).edge(bq, c).edge(c, a)
        out.append(case(name, b, idx, dict(F=3, nodes=3, **cl)))
    # 64 / 65 distinct query residues with a vote in one component (the best-target table has a lane each): a one-way path whose k-th edge is entered as
    # (2k, 2k + 1); the 33rd edge as (64, 0)
    for nq_ in (WAVE, WAVE + 1):
        p = _path(T, 34, two_way=False)
        b = MapBuilder(T)
        for k in range(32):
            b.edge(p[k], p[k + 1], qi=2 * k, qj=2 * k + 1)
        if nq_ > WAVE:
            b.edge(p[32], p[33], qi=64, qj=0)
        out.append(case("q_residues%d" % nq_, b, list(range(64)), dict(q_residues=nq_)))
        out[-1].path = "device" if nq_ <= WAVE else "overflow"
    # u8 saturation, as a host-path case (more than 64 nodes: the device glue declines): in a 200-residue structure the two residues with the most
    # neighbours, lo < hi, are both voted for query residue lo — hi by all its pairs in both directions, lo by 132 neighbours in both directions: fewer
    # votes than hi, more than 255.  Both counts stop at 255, the tie goes to the smaller residue lo; without the saturation hi would win
    T2 = base(200)
    deg = T2.valid.sum(axis=1)
    lo, hi = sorted(np.argsort(-deg, kind="stable")[:2].tolist())
    b, have = MapBuilder(T2), set()
    for ctr, nb in ((hi, [j for j in range(T2.n) if T2.valid[hi, j]]), (lo, [j for j in range(T2.n) if T2.valid[lo, j]][:132])):
        for j in nb:
            for u, v, qi, qj in ((ctr, j, lo, j), (j, ctr, j, lo)):
                h = T2.h(u, v)
                if h is not None and h not in have and j not in (lo, hi):
                    have.add(h)
                    b.edge(u, v, qi=qi, qj=qj)
    out.append(Case("saturation", "votes", T2, b.arrays(_fill_indices(T2, [lo, hi], 40)), dict(max_vote=255, sat_winner=True, winner=(lo, lo)), path="overflow"))
    # the host glue's own switches (fd_retrieve_host.cpp): more than HOST_DENSE found triples in a slot whose q_size x residues table is small -> the dense
    # (q, r) vote table instead of the hash map; more than HOST_DENSE hashes -> the hash -> entry table instead of bisection.  The first 4096 / 4097 pairs of
    # the 200-residue structure with a hash of their own, by identity; every edge brings its observed distance, so 4097 is a two-scan call as well
    pairs = [(i, j) for i in range(T2.n) for j in range(T2.n) if T2.uniq(i, j)]
    for F in (HOST_DENSE, HOST_DENSE + 1):
        b = MapBuilder(T2)
        for i, j in pairs[:F]:
            b.edge(i, j)
        out.append(Case("dense%d" % F, "votes", T2, b.arrays(list(range(8))), dict(F=F, hashes=F, n_aad=F, max_nodes=T2.n),
                        path="overflow" if F <= TWO_PASS_AAD else "host", targets=[T2]))
    return out


def _rescue_base(T, chain):
    """a two-way chain over `chain` (all assigned by identity)"""
    b = MapBuilder(T)
    for u, v in zip(chain, chain[1:]):
        b.edge(u, v).edge(v, u)
    return b


def _tune(T, b, indices, cutoff, metric, target, fill_q, partners=None):
    """observed distances of further pairs for query residue fill_q (one that is assigned: no rescue looks at them) until metric(model) == target"""
    def value():
        a = b.arrays(indices)
        f, c = model_scan(T, a, cutoff)
        return metric(f, c, a)
    cur = value()
    assert cur <= target, (cur, target)
    for i in range(T.n):
        for j in (partners if partners is not None else range(T.n)):
            if cur == target:
                return b
            if i == j or not T.valid[i, j]:
                continue
            b.obs(i, j, fill_q)
            v = value()
            if v > target or v == cur:
                b.aad.pop()
            else:
                cur = v
    assert cur == target, (cur, target)
    return b


def _tune_tally(T, b, indices, cutoff, target, q, assigned):
    """observed distances (i, p) with p assigned, tagged with the unmatched query residue q itself, until the rescue of q tallies exactly `target`
    candidate pairs (pairs of q whose partner is assigned); an entry's share is counted by a scan of that entry alone"""
    def count(aad):
        a = dict(b.arrays(indices))
        a["aad_aa1"], a["aad_aa2"] = np.array([x[0] for x in aad], np.uint8), np.array([x[1] for x in aad], np.uint8)
        a["aad_dist"], a["aad_qi"] = np.array([x[2] for x in aad], np.float32), np.array([x[3] for x in aad], np.uint32)
        c = model_scan(T, a, cutoff)[1]
        return int(((c[:, 0] == q) & np.isin(c[:, 2], assigned)).sum())
    cur = count(b.aad)
    for i in range(T.n):
        for p in assigned:
            if cur == target:
                return b
            if i == p or not T.valid[i, p]:
                continue
            e = (int(T.aa[i]), int(T.aa[p]), np.float32(T.D[i, p]), q)
            inc = count([e])
            if 0 < inc <= target - cur:
                b.aad.append(e)
                cur += inc
    assert cur == target, (cur, target)
    return b


def _rescuable(T, chain, k, need=2, order=None):
    """k residues outside `chain` that the scan can reach for a rescue: a residue type some hash of the chain carries (the prefilter of maps with at most
    200 hashes scans no other residue) and at least `need` chain residues within the 20 A cutoff"""
    types = {int(T.aa[p]) for p in chain}
    out = [x for x in (order if order is not None else range(T.n)) if x not in chain and int(T.aa[x]) in types and sum(bool(T.valid[x, p]) for p in chain) >= need]
    assert len(out) >= k
    return out[:k]


def _rescue_cases():
    T = base(120)
    chain = _small(T, 4, lo=30)
    p0, p1, p2, p3 = chain
    t, t2 = _rescuable(T, chain, 2, need=4)
    out = []

    def case(name, b, claims, idx=None, cutoff=0.01):
        return Case(name, "rescue", T, b.arrays([p0, p1, p2, p3, t] if idx is None else idx), claims, cutoff=cutoff)
    # a narrow window (0.01 A) keeps chance votes out of the small cases: the tallies (largest, residues holding it, taken) are the ones written here
    out.append(case("max_one", _rescue_base(T, chain).obs(t, p0, t), dict(tally=(1, 1, False), rescued=False)))
    out.append(case("unique_two", _rescue_base(T, chain).obs(t, p0, t).obs(t, p1, t), dict(tally=(2, 1, False), rescued=True)))
    out.append(case("tied_two", _rescue_base(T, chain).obs(t, p0, t).obs(t, p1, t).obs(t2, p2, t).obs(t2, p3, t), dict(tally=(2, 2, False), rescued=False)))
    out.append(case("unique_taken", _rescue_base(T, chain).obs(p0, p1, t).obs(p0, p2, t), dict(tally=(2, 1, True), rescued=False)))
    out.append(case("no_observed_distance", _rescue_base(T, chain), dict(tally=None, rescued=False)))
    # C candidate pairs in the slot, the rescue decided by pairs of residue tl: taken from the structure's end, so that they are among the slot's last
    chain = _path(T, 12)
    tl = _rescuable(T, chain, 1, need=4, order=range(T.n - 1, -1, -1))[0]
    ps = [p for p in chain if T.valid[tl, p]][:4]
    assert len(ps) == 4          # a tally of four: chance votes of other residues (same type, similar distance) reach two at most
    for C_ in (RS_CAND_LDS - 1, RS_CAND_LDS, RS_CAND_LDS + 1):
        b = _rescue_base(T, chain)
        for p in ps:
            b.obs(tl, p, tl)
        _tune(T, b, chain + [tl], 1.0, lambda f, c, a: len(c), C_, chain[0])
        out.append(Case("C%d" % C_, "rescue", T, b.arrays(chain + [tl]), dict(C=C_, rescued=True, rescue_row_from=RS_CAND_LDS - 64)))
    for n in (RS_S_FILT - 1, RS_S_FILT, RS_S_FILT + 1):
        b = _rescue_base(T, chain)
        for p in ps:
            b.obs(tl, p, tl)
        _tune(T, b, chain + [tl], 1.0, lambda f, c, a: int(np.isin(c[:, 2], chain).sum()), n, chain[0], partners=chain)
        out.append(Case("filt%d" % n, "rescue", T, b.arrays(chain + [tl]), dict(filt=n, rescued=True)))
    # the rescue's own list of voting pairs (n_t: pairs of the unmatched residue whose partner is assigned).  Split form: RS_S_LIST in the unfiltered walk
    # (more than RS_S_FILT pairs with an assigned partner) — one pair more overflows there and nowhere else
    for n in (RS_S_LIST - 1, RS_S_LIST, RS_S_LIST + 1):
        b = _rescue_base(T, chain)
        for p in ps:
            b.obs(tl, p, tl)
        _tune_tally(T, b, chain + [tl], 3.0, n, tl, chain)
        out.append(Case("tally%d" % n, "rescue", T, b.arrays(chain + [tl]), dict(tally_len=n, min_filt=RS_S_FILT + 1), cutoff=3.0,
                        path="overflow" if n > RS_S_LIST else "device", split_only=n > RS_S_LIST))
    # k_rs_slots: RS_LIST_CAP, in a slot of more than RS_S_EDGE found triples (which the split form hands to k_rs_slots)
    res = _central(T, 20)
    pairs = [(i, j) for i in res for j in res if T.uniq(i, j)]
    rng = np.random.Generator(np.random.PCG64(SEED + 20))
    pairs = [pairs[x] for x in rng.permutation(len(pairs))][:RS_S_EDGE + 1]
    tb = _rescuable(T, res, 1, need=4, order=range(T.n - 1, -1, -1))[0]
    for n in (RS_LIST_CAP - 1, RS_LIST_CAP, RS_LIST_CAP + 1):
        b = MapBuilder(T)
        for i, j in pairs:
            b.edge(i, j)
        _tune_tally(T, b, res + [tb], 3.0, n, tb, res)
        out.append(Case("tally%d" % n, "rescue", T, b.arrays(res + [tb]), dict(tally_len=n, F=RS_S_EDGE + 1), cutoff=3.0, path="overflow" if n > RS_LIST_CAP else "device",
                        targets=[T, base(120, SEED + 1)]))          # (the noisy copy would keep ~2,000 voting pairs with fewer than 129 found triples: the split form's cap)
    return out


def _filler_hashes(T, n):
    """n hashes that no pair of T carries (taken from another structure: real residue types in both fields)"""
    other = base(120, SEED + 1)
    ii, jj = np.nonzero(other.valid)
    have = set(T.hash_count)
    out = []
    for i, j in zip(ii.tolist(), jj.tolist()):
        h = other.h(i, j)
        if h is not None and h not in have:
            have.add(h)
            out.append(h)
            if len(out) == n:
                return out
    raise AssertionError("not enough filler hashes")


def _sizes_cases():
    T = base(120)
    r = _small(T, 3, lo=50)
    r = r + _rescuable(T, r, 1, need=3)
    out = []

    def graph():
        b = MapBuilder(T).edge(r[0], r[1]).edge(r[1], r[0]).edge(r[1], r[2])
        return b.obs(r[3], r[0], r[3]).obs(r[3], r[1], r[3])          # r[3] is rescued in both components
    for n in (63, 64, 65):
        out.append(Case("indices%d" % n, "sizes", T, graph().arrays(_fill_indices(T, r[:4], n)), dict(n_indices=n, comps=2, rescued=True), path="device" if n <= WAVE else "host"))
    for n in (PREFILTER, PREFILTER + 1, SETUP_HASH_LDS, SETUP_HASH_LDS + 1, MP_QH_LDS, MP_QH_LDS + 1, RS_LIST_CAP, RS_LIST_CAP + 1):
        b = graph()
        fill = _filler_hashes(T, n - 3)
        for k, h in enumerate(fill):          # the three real hashes end up spread over the sorted set; filler entries between the real ones
            b.ent.insert(1 + (k % 3), (h, r[k % 3], r[(k + 1) % 3], np.float32(1.0 / 256.0)))
        out.append(Case("hashes%d" % n, "sizes", T, b.arrays(r[:4]), dict(hashes=n, comps=2, rescued=True)))
    for n in (AAD_SORTED, AAD_SORTED + 1, MP_AAD_LDS, MP_AAD_LDS + 1, TWO_PASS_AAD, TWO_PASS_AAD + 1):
        b = graph()
        real = b.aad
        k = n - len(real)
        # filler: every residue-type pair in turn, distances the target does not have (beyond the 20 A cutoff by more than any window)
        fill = [(x % 20, (x // 20) % 20, np.float32(30.0 + 0.001 * x), r[x % 4]) for x in range(k)]
        step = max(1, k // len(real))
        b.aad = []
        for x in range(k):
            if x % step == 0 and real:
                b.aad.append(real.pop(0))
            b.aad.append(fill[x])
        b.aad += real
        out.append(Case("aad%d" % n, "sizes", T, b.arrays(r[:4]), dict(n_aad=n, comps=2, rescued=True), path="device" if n <= TWO_PASS_AAD else "host"))
    return out


def _window_cases():
    T = base(120)
    r = _small(T, 4, lo=70)
    out = []
    # a pair with 8 <= d < 13: d - c and d + c are exact in f32 for every cutoff used (d + 3 stays below 16, d - 3 lies on a finer grid)
    i, j = next((i, j) for i in range(T.n) for j in range(T.n) if T.uniq(i, j) and T.uniq(j, i) and 8.0 <= T.D[i, j] < 13.0)
    d = np.float32(T.D[i, j])
    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    dn = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))

    def edge_entries(b, c):
        """six observed distances for the pair (i, j), tagged with query residues 1 .. 6: below d one ulp inside / on / outside the window, above d the same"""
        c = np.float32(c)
        lo, hi = np.float32(d - c), np.float32(d + c)
        assert np.float32(d - lo) == c and np.float32(hi - d) == c          # both ends are exact in f32
        for tag, x in enumerate((up(lo), lo, dn(lo), dn(hi), hi, up(hi)), start=1):
            b.raw_obs(int(T.aa[i]), int(T.aa[j]), x, tag)
        return b
    for c in (1.0, 1.5, 3.0):
        b = MapBuilder(T).edge(i, j, obs=False).edge(j, i)
        edge_entries(b, c)
        out.append(Case("ulp_%g" % c, "window", T, b.arrays([i, j]), dict(pair=(i, j), tags_passing=[1, 4]), cutoff=c))
    for name, c in (("cutoff_zero", 0.0), ("cutoff_nan", float("nan"))):
        b = MapBuilder(T).edge(i, j).edge(j, i)
        out.append(Case(name, "window", T, b.arrays([i, j]), dict(F=0, C=0, comps=0), cutoff=c))
    b = MapBuilder(T).edge(i, j).edge(j, i)
    for a1, a2 in ((20, 3), (3, 31), (32, 3), (3, 33), (255, 255), (int(T.aa[i]), 255), (32 + int(T.aa[i]), int(T.aa[j]))):
        b.raw_obs(a1, a2, d, 7)
    out.append(Case("residue_types", "window", T, b.arrays([i, j]), dict(F=2, comps=1, tags_absent=[7])))
    # beyond MP_AAD_LDS entries the scan merges the windows of one type pair into float intervals: windows of (aa[i], aa[j]) that overlap, abut and leave a gap,
    # with the pair's distance d on the open end of one (exactly on: no pass), inside the overlap, and in the gap
    c = np.float32(1.0)
    for name, xs, passing in (("merged_overlap", (d - c, d + np.float32(0.5)), [2]), ("merged_abut", (d - c, d + c), []),
                              ("merged_gap_inside", (up(d - c), d + np.float32(2.5)), [1])):
        b = MapBuilder(T).edge(i, j, obs=False).edge(j, i)
        for tag, x in enumerate(xs, start=1):
            b.raw_obs(int(T.aa[i]), int(T.aa[j]), x, tag)
        k = 0
        while len(b.aad) < MP_AAD_LDS + 76:
            b.raw_obs(k % 20, (k // 20) % 20, np.float32(2.0 + 0.37 * (k % 47)), r[2 + k % 2])
            k += 1
        out.append(Case(name, "window", T, b.arrays([i, j, r[2], r[3]]), dict(pair=(i, j), tags_passing=passing, n_aad=MP_AAD_LDS + 76)))
    return out


def _long_cases():
    out = []
    for n in (64 * MP_SCAN_BLOCKS, 64 * MP_SCAN_BLOCKS + 1):
        T = base(n)
        b = MapBuilder(T)
        near = [x for x in range(n - 1, n - 40, -1) if T.h(0, x) is None and T.h(n - 1, x) is not None][:2]
        lo = [x for x in range(1, 40) if T.h(0, x) is not None][:2]
        for u, v in ((0, lo[0]), (lo[0], 0), (lo[0], lo[1]), (n - 1, near[0]), (near[0], n - 1), (near[0], near[1])):
            if T.h(u, v) is not None:
                b.edge(u, v)
        out.append(Case("residues%d" % n, "long", T, b.arrays([0, lo[0], lo[1], n - 1, near[0], near[1]]), dict(residues=n, min_comps=2), targets=[T]))
    return out


@functools.lru_cache(maxsize=None)
def cases(cls):
    return {"nodes": _nodes_cases, "edges": _edges_cases, "comps": _comps_cases, "votes": _votes_cases, "rescue": _rescue_cases, "sizes": _sizes_cases,
            "window": _window_cases, "long": _long_cases}[cls]()


# ---------------------------------------------------------------------------------------------------------------- the oracle's answer, once per case
_ORACLE = {}


def oracle_results(c):
    """oracle.retrieve of every target of the case, computed once and shared (the tests leave it unchanged)"""
    key = (c.cls, c.name)
    if key not in _ORACLE:
        m = oracle_map(c.arrays)
        _ORACLE[key] = [oracle.retrieve(t.o, c.query.o, m, node_count=c.node_count, ca_distance_cutoff=c.ca_distance_cutoff) for t in c.targets]
    return _ORACLE[key]
