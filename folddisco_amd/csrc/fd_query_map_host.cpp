// fd_query_map_host.cpp — the host part of make_query_map (see fd_query_map_host.h).  Host C++ alone.  The only arithmetic here that decides a hash bit
// is the expansion's feature +- threshold: single IEEE f32 adds in the reference's order (the library builds with -ffp-contract=off).
#include "fd_query_map_host.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <map>
#include <unordered_set>
#include <utility>

void qm_run_parts(fd_host_pool *pool, unsigned threads, unsigned n, const std::function<void(unsigned)> &part) {
    std::atomic<unsigned> next(0);
    const std::function<void()> worker = [&]() { for (;;) { const unsigned z = next.fetch_add(1); if (z >= n) break; part(z); } };
    if (pool) pool->run(threads, worker);
    else worker();
}

// ---------------------------------------------------------------------------------------------------------------------- pairs
void qm_list_pairs(uint64_t n_queries, const uint32_t *q_struct, const uint64_t *q_off, const uint32_t *q_index, const uint64_t *res_off, qm_pairs &P) {
    // (a whole-structure query lists ~10^5 pairs: the arrays are sized once and written through pointers — growing them by doubling and two
    // push_backs per pair were most of this stage)
    uint64_t n_pairs_max = 0;
    for (uint64_t t = 0; t < n_queries; ++t) { const uint64_t n_q = q_off[t + 1] - q_off[t]; n_pairs_max += n_q * (n_q ? n_q - 1 : 0); }
    P.pi.resize(n_pairs_max); P.pj.resize(n_pairs_max);
    P.off.assign(n_queries + 1, 0);
    uint32_t *wi = P.pi.data(), *wj = P.pj.data();
    size_t w = 0;
    for (uint64_t t = 0; t < n_queries; ++t) {
        const uint64_t r0 = res_off[q_struct[t]], R = res_off[q_struct[t] + 1] - r0;
        const uint32_t *qi = q_index + q_off[t];
        const uint64_t n_q = q_off[t + 1] - q_off[t];
        for (uint64_t a = 0; a < n_q; ++a) {
            if (!(qi[a] < R)) continue;
            const uint32_t ra = (uint32_t)(r0 + qi[a]);
            for (uint64_t b = 0; b < n_q; ++b)
                if (a != b && qi[b] < R) { wi[w] = ra; wj[w] = (uint32_t)(r0 + qi[b]); ++w; }
        }
        P.off[t + 1] = w;
    }
    P.pi.resize(w); P.pj.resize(w);
}

// --------------------------------------------------------------------------------------------------------------------- fields
// dist_index / angle_index of the encoding (controller/feature.rs:269-291): theta only for the two PDBMotif forms — and PDBMotif shifts its
// DEGREE-valued theta by the threshold converted to radians, like the reference.  Substitutions touch the residue fields of the container:
// encodings without them take none (amino_acid_index, controller/feature.rs:260-267)
qm_fields qm_fields_of(uint32_t hash_type) {
    switch (hash_type) {
        case 0: case 1: return {{2, 3}, 2, {4}, 1, true};                          // PDBMotif, PDBMotifSinCos
        case 2: return {{2}, 1, {3, 4, 5, 6, 7}, 5, true};                         // TrRosetta
        case 4: return {{2}, 1, {3, 4, 5}, 3, true};                               // PointPairFeature
        case 5: return {{7}, 1, {0, 1, 2, 3, 4, 5, 6}, 7, false};                  // TertiaryInteraction
        case 6: return {{2, 3}, 2, {4, 5, 6, 7, 8}, 5, false};                     // Hybrid
        default: return {{2, 3}, 2, {4, 5, 6}, 3, true};                           // PDBTrRosetta, FolddiscoAngle, FolddiscoDist
    }
}

// ------------------------------------------------------------------------------------------------------------- observed lists
// observed (aa_i, aa_j, CA distance) list (structure/core.rs:462-477: distance <= 20.0)
static void qm_observed_range(const qm_feat &F, const uint32_t *pi, uint64_t ka, uint64_t kb, uint64_t r0, qm_aad &A) {
    A.a1.reserve(A.a1.size() + (kb - ka)); A.a2.reserve(A.a2.size() + (kb - ka)); A.ad.reserve(A.ad.size() + (kb - ka)); A.aq.reserve(A.aq.size() + (kb - ka));
    for (uint64_t k = ka; k < kb; ++k) {
        if (!F.valid[k]) continue;
        const float *f = &F.feat[(size_t)FD_QF * k];
        if (f[9] <= 20.0f) { A.a1.push_back((uint8_t)f[10]); A.a2.push_back((uint8_t)f[11]); A.ad.push_back(f[9]); A.aq.push_back((uint32_t)(pi[k] - r0)); }
    }
}
void qm_observed_list(const qm_feat &F, const uint32_t *pi, uint64_t k0, uint64_t k1, uint64_t r0, fd_host_pool *pool, unsigned threads, qm_aad &A) {
    if (!pool) { qm_observed_range(F, pi, k0, k1, r0, A); return; }
    // a whole-structure query: the list is read from the page-locked landing block (a cache miss per pair: the copy engine wrote it) — eight
    // parts on the helper threads, joined in pair order
    constexpr unsigned NP = 8;
    qm_aad part[NP];
    qm_run_parts(pool, threads, NP, [&](unsigned z) {
        qm_aad P;              // (a local: the parts' vector headers share cache lines)
        qm_observed_range(F, pi, k0 + (k1 - k0) * z / NP, k0 + (k1 - k0) * (z + 1) / NP, r0, P);
        part[z] = std::move(P);
    });
    A.a1.reserve(k1 - k0); A.a2.reserve(k1 - k0); A.ad.reserve(k1 - k0); A.aq.reserve(k1 - k0);
    for (unsigned z = 0; z < NP; ++z) {
        A.a1.insert(A.a1.end(), part[z].a1.begin(), part[z].a1.end()); A.a2.insert(A.a2.end(), part[z].a2.begin(), part[z].a2.end());
        A.ad.insert(A.ad.end(), part[z].ad.begin(), part[z].ad.end()); A.aq.insert(A.aq.end(), part[z].aq.begin(), part[z].aq.end());
    }
}

// ------------------------------------------------------------------------------------------------------------------ expansion
namespace {
struct qm_sub { const uint8_t *aa; uint32_t n; };
struct qm_pair_ref { uint32_t qi, qj, pair; };
}
static void qm_push(qm_cands &C, const float *f, const qm_pair_ref &r, bool primary) {
    C.vf.insert(C.vf.end(), f, f + FD_QF);
    C.c.push_back({r.qi, r.qj, (uint8_t)(primary ? 1 : 0), r.pair});
}
static void qm_push_sub(qm_cands &C, const float *f, const qm_pair_ref &r, int field0, float v0, int field1, float v1) {
    float t[FD_QF];
    memcpy(t, f, sizeof t);
    t[field0] = v0;
    if (field1 >= 0) t[field1] = v1;
    qm_push(C, t, r, false);
}
// apply_substitutions (query.rs:86-156): i alone, then i x j (a x b order) when both have a list; j alone only without a list for i
static void qm_substitute(qm_cands &C, const float *f, const qm_pair_ref &r, const qm_sub *si, const qm_sub *sj) {
    if (si) {
        for (uint32_t a = 0; a < si->n; ++a) qm_push_sub(C, f, r, 0, (float)si->aa[a], -1, 0.f);
        if (sj)
            for (uint32_t a = 0; a < si->n; ++a)
                for (uint32_t b = 0; b < sj->n; ++b) qm_push_sub(C, f, r, 0, (float)si->aa[a], 1, (float)sj->aa[b]);
    } else if (sj)
        for (uint32_t b = 0; b < sj->n; ++b) qm_push_sub(C, f, r, 1, (float)sj->aa[b], -1, 0.f);
}
// expand_and_insert (query.rs:179-206) over one group of fields
static void qm_expand_group(qm_cands &C, float *near, float *far, const qm_pair_ref &r, const int *idxs, int n_idx, const float *thr, uint64_t n_thr) {
    for (uint64_t z2 = 0; z2 < n_thr; ++z2)
        for (int z = 0; z < n_idx; ++z) {
            const int idx = idxs[z];
            near[idx] = near[idx] - thr[z2];
            far[idx] = far[idx] + thr[z2];
            qm_push(C, near, r, false);
            qm_push(C, far, r, false);
            // the reference restores with += / -= (f32, not an exact inverse): keep the drift
            near[idx] = near[idx] + thr[z2];
            far[idx] = far[idx] - thr[z2];
        }
}
void qm_expand_query(const qm_feat &F, const uint32_t *pi, const uint32_t *pj, uint64_t k0, uint64_t k1, uint64_t r0, const uint32_t *qidx, uint64_t n_q,
                     const uint8_t *const *subs, const uint32_t *n_subs, const qm_fields &fl, const qm_thresholds &T, qm_cands &C) {
    // substitution map keyed by residue index: a later entry for the same residue overrides (query.rs:236-246)
    std::map<uint32_t, qm_sub> sub_of;
    if (subs && n_subs && fl.has_aa)
        for (uint64_t a = 0; a < n_q; ++a)
            if (subs[a]) sub_of[qidx[a]] = qm_sub{subs[a], n_subs[a]};
    for (uint64_t k = k0; k < k1; ++k) {
        if (!F.valid[k]) continue;
        const float *f = &F.feat[(size_t)FD_QF * k];
        const qm_pair_ref r = {(uint32_t)(pi[k] - r0), (uint32_t)(pj[k] - r0), (uint32_t)k};
        qm_push(C, f, r, true);
        float near[FD_QF], far[FD_QF];
        memcpy(near, f, sizeof near);
        memcpy(far, f, sizeof far);
        const auto si = sub_of.find(r.qi), sj = sub_of.find(r.qj);
        qm_substitute(C, near, r, si != sub_of.end() ? &si->second : nullptr, sj != sub_of.end() ? &sj->second : nullptr);
        qm_expand_group(C, near, far, r, fl.di, fl.ndi, T.dist, T.n_dist);
        qm_expand_group(C, near, far, r, fl.ai, fl.nai, T.angle_rad, T.n_angle);
    }
}

// ----------------------------------------------------------------------------------------------------------- first insertions
// a motif query's few hundred insertions: a small open-addressing table (a node-based set cost 3x this)
static void qm_first_table(const qm_insertions &I, std::vector<uint64_t> &tab, std::vector<uint32_t> &keep) {
    uint32_t cap = 64;
    while (cap < 2 * I.n_ins) cap <<= 1;
    tab.assign(cap, ~0ull);
    keep.reserve((size_t)I.n_ins);
    const uint32_t *h1 = I.n_planes == 1 ? I.planes[0] + I.c0 : nullptr;       // one bin configuration: position = candidate (no division per insertion)
    for (uint64_t pos = 0; pos < I.n_ins; ++pos) {
        const uint32_t h = h1 ? h1[pos] : qm_hash_at(I, pos);
        uint32_t at = (h * 2654435761u) & (cap - 1);
        while (tab[at] != ~0ull && (uint32_t)tab[at] != h) at = (at + 1) & (cap - 1);
        if (tab[at] == ~0ull) { tab[at] = h; keep.push_back((uint32_t)pos); }
    }
}
// many insertions (whole-structure queries, ~10^5): (hash << 32 | insertion position) keys through an LSD radix sort, first key of every hash
// kept, survivors back in insertion order — a third of a hash set's time there
static void qm_first_radix(const qm_insertions &I, std::vector<uint32_t> &keep) {
    const uint64_t n = I.n_ins;
    std::vector<uint64_t> key(n), tmp(n);
    for (uint64_t pos = 0; pos < n; ++pos) key[pos] = ((uint64_t)qm_hash_at(I, pos) << 32) | pos;
    for (int pass = 0; pass < 4; ++pass) {
        const int sh = 32 + 8 * pass;
        size_t cnt[257] = {0};
        for (uint64_t k = 0; k < n; ++k) ++cnt[((key[k] >> sh) & 255u) + 1];
        for (int d = 0; d < 256; ++d) cnt[d + 1] += cnt[d];
        for (uint64_t k = 0; k < n; ++k) tmp[cnt[(key[k] >> sh) & 255u]++] = key[k];
        key.swap(tmp);
    }
    std::vector<uint8_t> first(n, 0);      // the stable sort left every hash's earliest insertion first: mark, then walk in order
    for (uint64_t k = 0; k < n; ++k) if (k == 0 || (key[k] >> 32) != (key[k - 1] >> 32)) first[(uint32_t)key[k]] = 1;
    for (uint64_t pos = 0; pos < n; ++pos) if (first[pos]) keep.push_back((uint32_t)pos);
}
static void qm_first_set(const qm_insertions &I, std::vector<uint32_t> &keep) {
    std::unordered_set<uint32_t> have;
    have.reserve((size_t)I.n_ins / 4 + 16);
    for (uint64_t pos = 0; pos < I.n_ins; ++pos) if (have.insert(qm_hash_at(I, pos)).second) keep.push_back((uint32_t)pos);
}
void qm_first_wins(const qm_insertions &I, std::vector<uint64_t> &tab, std::vector<uint32_t> &keep, uint64_t table_max, uint64_t set_min) {
    if (I.n_ins <= table_max) qm_first_table(I, tab, keep);
    else if (I.n_ins >= set_min) qm_first_set(I, keep);
    else qm_first_radix(I, keep);
}

// ------------------------------------------------------------------------------------------------------------ arena and fill
qm_arena qm_arena_layout(size_t n, size_t n_idx, size_t n_aad, bool with_post) {
    const auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    qm_arena L;
    L.hash = up16(sizeof(fd_query_map)); L.qi = L.hash + up16(n * 4); L.qj = L.qi + up16(n * 4); L.idf = L.qj + up16(n * 4); L.ph = L.idf + up16(n * 4);
    L.pl = L.ph + up16(n * 4); L.pk = L.pl + (with_post ? up16(n * 8) : 0); L.ps = L.pk + (with_post ? up16(n * 8) : 0);
    L.idx = L.ps + (with_post ? up16(n * 4) : 0); L.ad = L.idx + up16(n_idx * 4); L.aq = L.ad + up16(n_aad * 4); L.prim = L.aq + up16(n_aad * 4);
    L.a1 = L.prim + up16(n); L.a2 = L.a1 + up16(n_aad); L.bytes = L.a2 + up16(n_aad) + 16;
    return L;
}
// entries [a, b) of a device form's map.  Kept positions ascend: the pair a position belongs to advances with them (no division per entry)
static void qm_fill_implied(const qm_map_src &S, fd_query_map *m, size_t a, size_t b) {
    if (a >= b) return;
    const uint32_t *hashes = S.ins.planes[0];
    const uint64_t pp = S.per_pair;
    uint64_t v = (S.ins.c0 + S.keep[a]) / pp, v_end = (v + 1) * pp;      // candidates of valid pair v: [v * pp, v_end)
    for (size_t e = a; e < b; ++e) {
        const uint64_t z = S.ins.c0 + S.keep[e];
        while (z >= v_end) { ++v; v_end += pp; }
        const uint32_t k = S.vpairs[v];
        m->hash[e] = hashes[z]; m->qi[e] = (uint32_t)(S.pi[k] - S.r0); m->qj[e] = (uint32_t)(S.pj[k] - S.r0); m->is_primary[e] = z + pp == v_end ? 1 : 0;
        m->idf[e] = S.pair_idf[k]; m->primary_hash[e] = S.pair_primary[k];
    }
}
static void qm_fill_stored(const qm_map_src &S, fd_query_map *m) {
    for (size_t e = 0; e < S.n; ++e) {
        const qm_cand &cz = S.cands[S.ins.c0 + S.keep[e] / S.ins.n_planes];
        m->hash[e] = qm_hash_at(S.ins, S.keep[e]); m->qi[e] = cz.qi; m->qj[e] = cz.qj; m->is_primary[e] = cz.primary;
        m->idf[e] = S.pair_idf[cz.pair]; m->primary_hash[e] = S.pair_primary[cz.pair];
    }
}
fd_query_map *qm_fill_map(const qm_map_src &S, fd_host_pool *pool, unsigned threads) {
    const size_t n = S.n, n_aad = S.aad->ad.size();
    const bool with_post = S.post_len && n;
    const qm_arena L = qm_arena_layout(n, S.n_idx, n_aad, with_post);
    uint8_t *blk = (uint8_t *)malloc(L.bytes);
    if (!blk) return nullptr;
    fd_query_map *m = (fd_query_map *)blk;
    memset(m, 0, sizeof *m);
    m->arena_bytes = L.bytes;
    m->n = n;
    m->hash = (uint32_t *)(blk + L.hash); m->qi = (uint32_t *)(blk + L.qi); m->qj = (uint32_t *)(blk + L.qj); m->idf = (float *)(blk + L.idf);
    m->primary_hash = (uint32_t *)(blk + L.ph); m->is_primary = blk + L.prim;
    if (S.cands) qm_fill_stored(S, m);
    else if (n < QM_PARTS_MIN) qm_fill_implied(S, m, 0, n);
    else       // a whole-structure query's ~10^5 entries: eight parts on the helper threads (0.5 ms of the call on one)
        qm_run_parts(pool, threads, 8, [&](unsigned z) { qm_fill_implied(S, m, n * z / 8, n * (z + 1) / 8); });
    if (with_post) {
        m->post_len = (uint64_t *)(blk + L.pl); m->post_kidx = (long long *)(blk + L.pk); m->post_seg = (uint32_t *)(blk + L.ps);
        memcpy(m->post_len, S.post_len, n * 8); memcpy(m->post_seg, S.post_seg, n * 4); memcpy(m->post_kidx, S.post_kidx, n * 8);
        m->post_index_uid = S.index_uid;
    }
    m->n_indices = S.n_idx; m->indices = (uint32_t *)(blk + L.idx);
    if (S.n_idx) memcpy(m->indices, S.indices, S.n_idx * 4);
    m->n_aad = n_aad; m->aad_dist = (float *)(blk + L.ad); m->aad_qi = (uint32_t *)(blk + L.aq); m->aad_aa1 = blk + L.a1; m->aad_aa2 = blk + L.a2;
    if (n_aad) { memcpy(m->aad_dist, S.aad->ad.data(), n_aad * 4); memcpy(m->aad_qi, S.aad->aq.data(), n_aad * 4); memcpy(m->aad_aa1, S.aad->a1.data(), n_aad); memcpy(m->aad_aa2, S.aad->a2.data(), n_aad); }
    return m;
}

// ---- test-only entries (include/fdgpu_debug.h): no context, no device ----------------------------------------------------
template <typename T> static T *qm_dup(const T *v, size_t n) {
    T *p = (T *)malloc(std::max<size_t>(n, 1) * sizeof(T));
    if (p && n) memcpy(p, v, n * sizeof(T));
    return p;
}
extern "C" int fdgpu_debug_qm_pairs(uint64_t n_queries, const uint32_t *q_struct, const uint64_t *q_off, const uint32_t *q_index, const uint64_t *res_off,
                                    uint32_t **pair_i, uint32_t **pair_j, uint64_t *pair_off) {
    if (!q_off || !res_off || !pair_i || !pair_j || !pair_off || (n_queries && !q_struct) || (q_off[n_queries] && !q_index)) return FDGPU_EINVAL;
    qm_pairs P;
    qm_list_pairs(n_queries, q_struct, q_off, q_index, res_off, P);
    memcpy(pair_off, P.off.data(), (n_queries + 1) * 8);
    *pair_i = qm_dup(P.pi.data(), P.pi.size()); *pair_j = qm_dup(P.pj.data(), P.pj.size());
    return *pair_i && *pair_j ? FDGPU_OK : FDGPU_ENOMEM;
}
extern "C" int fdgpu_debug_qm_fields(uint32_t hash_type, int32_t *out) {
    if (!out) return FDGPU_EINVAL;
    const qm_fields fl = qm_fields_of(hash_type);
    for (int z = 0; z < 12; ++z) out[z] = -1;
    out[0] = fl.ndi; out[3] = fl.nai; out[11] = fl.has_aa ? 1 : 0;
    for (int z = 0; z < fl.ndi; ++z) out[1 + z] = fl.di[z];
    for (int z = 0; z < fl.nai; ++z) out[4 + z] = fl.ai[z];
    return FDGPU_OK;
}
extern "C" int fdgpu_debug_qm_expand(const float *features, const uint8_t *valid, const uint32_t *pair_i, const uint32_t *pair_j, uint64_t n_pairs, uint64_t r0,
                                     const uint32_t *q_index, uint64_t n_q, const uint8_t *const *subs, const uint32_t *n_subs, uint32_t hash_type,
                                     const float *dist_thr, uint64_t n_dist, const float *angle_thr_rad, uint64_t n_angle, float **cand_features,
                                     uint32_t **cand_recs, uint64_t *n_cands) {
    if (!cand_features || !cand_recs || !n_cands || (n_pairs && (!features || !valid || !pair_i || !pair_j)) || (n_q && !q_index) || (n_dist && !dist_thr) ||
        (n_angle && !angle_thr_rad))
        return FDGPU_EINVAL;
    qm_cands C;
    qm_expand_query(qm_feat{features, valid}, pair_i, pair_j, 0, n_pairs, r0, q_index, n_q, subs, n_subs, qm_fields_of(hash_type),
                    qm_thresholds{dist_thr, n_dist, angle_thr_rad, n_angle}, C);
    std::vector<uint32_t> rec(4 * C.c.size());
    for (size_t z = 0; z < C.c.size(); ++z) { rec[4 * z] = C.c[z].qi; rec[4 * z + 1] = C.c[z].qj; rec[4 * z + 2] = C.c[z].primary; rec[4 * z + 3] = C.c[z].pair; }
    *n_cands = C.c.size();
    *cand_features = qm_dup(C.vf.data(), C.vf.size()); *cand_recs = qm_dup(rec.data(), rec.size());
    return *cand_features && *cand_recs ? FDGPU_OK : FDGPU_ENOMEM;
}
extern "C" int fdgpu_debug_qm_first_insertions(const uint32_t *hashes, uint64_t n_cands, uint32_t n_cfg, uint64_t table_max, uint64_t set_min, uint32_t **keep,
                                               uint64_t *n_keep) {
    if (!keep || !n_keep || (n_cands && !hashes) || n_cfg > 8) return FDGPU_EINVAL;
    const uint32_t n_planes = std::max(n_cfg, 1u);
    const uint32_t *planes[8];
    for (uint32_t k = 0; k < n_planes; ++k) planes[k] = hashes + (size_t)k * n_cands;
    std::vector<uint64_t> tab;
    std::vector<uint32_t> kept;
    qm_first_wins(qm_insertions{planes, n_planes, 0, n_cands * n_planes}, tab, kept, table_max ? table_max : QM_FI_TABLE_MAX, set_min ? set_min : QM_FI_SET_MIN);
    *n_keep = kept.size();
    *keep = qm_dup(kept.data(), kept.size());
    return *keep ? FDGPU_OK : FDGPU_ENOMEM;
}
extern "C" int fdgpu_debug_qm_arena(uint64_t n, uint64_t n_indices, uint64_t n_aad, uint32_t with_post, uint64_t *offsets) {
    if (!offsets) return FDGPU_EINVAL;
    const qm_arena L = qm_arena_layout(n, n_indices, n_aad, with_post != 0);
    const size_t o[15] = {L.hash, L.qi, L.qj, L.idf, L.ph, L.pl, L.pk, L.ps, L.idx, L.ad, L.aq, L.prim, L.a1, L.a2, L.bytes};
    for (int k = 0; k < 15; ++k) offsets[k] = o[k];
    return FDGPU_OK;
}
extern "C" int fdgpu_debug_qm_fill(const uint32_t *keep, uint64_t n, const uint32_t *hashes, uint64_t n_cands, uint32_t n_cfg, uint64_t c0, const uint32_t *cand_recs,
                                   const uint32_t *valid_pairs, uint64_t per_pair, const uint32_t *pair_i, const uint32_t *pair_j, uint64_t r0, const float *pair_idf,
                                   const uint32_t *pair_primary, const uint64_t *post_len, const uint32_t *post_seg, const long long *post_kidx, uint64_t index_uid,
                                   const uint32_t *indices, uint64_t n_indices, const uint8_t *aad_aa1, const uint8_t *aad_aa2, const float *aad_dist,
                                   const uint32_t *aad_qi, uint64_t n_aad, uint32_t pooled, fd_query_map **out) {
    if (!out || n_cfg > 8 || (n && (!keep || !hashes || !pair_idf || !pair_primary)) || (!cand_recs && n && (!valid_pairs || !per_pair || !pair_i || !pair_j || n_cfg)) ||
        (n_aad && (!aad_aa1 || !aad_aa2 || !aad_dist || !aad_qi)) || (n_indices && !indices))
        return FDGPU_EINVAL;
    const uint32_t n_planes = std::max(n_cfg, 1u);
    const uint32_t *planes[8];
    for (uint32_t k = 0; k < n_planes; ++k) planes[k] = hashes + (size_t)k * n_cands;
    std::vector<qm_cand> cands(cand_recs ? n_cands : 0);
    for (size_t z = 0; z < cands.size(); ++z) cands[z] = {cand_recs[4 * z], cand_recs[4 * z + 1], (uint8_t)cand_recs[4 * z + 2], cand_recs[4 * z + 3]};
    qm_aad A;
    A.a1.assign(aad_aa1, aad_aa1 + n_aad); A.a2.assign(aad_aa2, aad_aa2 + n_aad); A.ad.assign(aad_dist, aad_dist + n_aad); A.aq.assign(aad_qi, aad_qi + n_aad);
    const qm_map_src S = {keep, (size_t)n, qm_insertions{planes, n_planes, c0, 0}, cand_recs ? cands.data() : nullptr, valid_pairs, per_pair, pair_i, pair_j, r0, pair_idf,
                          pair_primary, post_len, post_seg, post_kidx, index_uid, indices, (size_t)n_indices, &A};
    fd_host_pool pool;
    *out = qm_fill_map(S, pooled ? &pool : nullptr, pooled ? 4 : 1);
    return *out ? FDGPU_OK : FDGPU_ENOMEM;
}
