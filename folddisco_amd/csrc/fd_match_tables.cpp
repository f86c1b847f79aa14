// fd_match_tables.cpp — the pair scan's host block (fd_match_tables.h): work items, per-query tables, interval tables, layout, packing.  Host C++ alone.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>
#include <utility>
#include "fd_match_tables.h"
#include "../../include/fdgpu_debug.h"
// the library's build hands every source to the HIP front end, where fd_libm.h marks its functions with a word of the HIP runtime header — which this
// file does not include; a plain host compiler (tools/check_match_tables.cpp's build) takes the header's other branch
#if defined(__HIPCC__) && !defined(__forceinline__)
#define __forceinline__ inline __attribute__((always_inline))
#endif
#include "fd_geom.h"      // fd_hash_aa_pair

#ifndef FD_WAVE            // fd_device.h defines it for the device side; a work item's i-tile is one wavefront of residues
#define FD_WAVE 64
#endif

// ---- work items ---------------------------------------------------------------------------------------------------------
// (query, candidate slot, 64-residue i-tile); a handful of long candidates (whole-structure queries: the top 20) would leave most of the chip idle,
// so the partner residues are split into spans as well until ~2000 wavefronts exist.
// many candidates (a batch of motif queries): spans of 256 partners cap the longest work items — the scan launch ends with its slowest wavefront, and a
// wavefront walks its partners one at a time (128 queries x 32 candidates, k_mp_scan: 93 us at 512, 68 at 256, 60 at 128 — where the drains, one per
// partly filled chunk, have grown by as much)
// large queries (whole-structure: the window test passes nearly every pair inside the cutoff, so a work item's time is its number of close
// pairs x one descriptor + hash each): while scan and drain were one kernel, a diagonal block of 64 x 128 residues was 128 drains on ONE wavefront and
// spans of 32 partners measured best (5.1 ms at 128, 4.4 at 64, 3.7 at 32).  With the drains in their own launch (k_mp_drain, a wavefront per chunk) the
// scan's work items only test and queue: 128 partners per item (first + second scan of the top 20 of a 300-residue query: 1.64 + 1.45 ms at 32,
// 1.32 + 1.19 at 64, 1.21 + 1.02 at 128, 1.24 + 1.00 at 256)
static uint32_t mp_j_span(uint64_t n_tiles, uint64_t max_aad) {
    return !n_tiles ? 0u : max_aad > 4096 ? 128u : n_tiles < 256 ? 64u : n_tiles < 1024 ? 128u : 256u;
}

int mp_work_items(const mp_tables_in &in, mp_items &W, const char **err) {
    const uint64_t n_cand = in.cand_off[in.n_queries];
    std::vector<uint64_t> len(n_cand);
    uint64_t n_tiles = 0, max_aad = 0;
    for (uint64_t k = 0; k < n_cand; ++k) {
        if (in.cand[k] >= in.n_struct) { *err = "match_pairs: candidate id outside the batch"; return FDGPU_EINVAL; }
        len[k] = in.res_off[in.cand[k] + 1] - in.res_off[in.cand[k]];
        n_tiles += (len[k] + FD_WAVE - 1) / FD_WAVE;
    }
    for (uint64_t t = 0; t < in.n_queries; ++t) max_aad = std::max<uint64_t>(max_aad, in.qs[t].n_aad);
    const uint32_t j_span = W.j_span = mp_j_span(n_tiles, max_aad);
    // a one-off block (a batch of motif queries: 18 k work items per 128 queries) gets its work items written on the DEVICE (k_mp_items): the host
    // sends every candidate's first item and query (8 bytes per candidate instead of 16 per item) and builds no item arrays
    if (in.dev_items) { W.wbase.resize(n_cand + 1); W.cq.resize(std::max<uint64_t>(n_cand, 1)); }
    size_t n_wi = 0;
    for (uint64_t k = 0; k < n_cand; ++k) {
        if (in.dev_items) W.wbase[k] = (uint32_t)n_wi;
        n_wi += ((len[k] + FD_WAVE - 1) / FD_WAVE) * (j_span ? (len[k] + j_span - 1) / j_span : (len[k] ? 1 : 0));
    }
    W.n_wi = n_wi;
    if (in.dev_items) {
        // (k_mp_items keeps a candidate's first entry of the active-residue list as the 32-bit word 64 x first item)
        if (n_wi >= (1ull << 26)) { *err = "match_pairs: more than 2^26 work items in one call; split the candidates"; return FDGPU_ERANGE; }
        W.wbase[n_cand] = (uint32_t)n_wi;
        for (uint64_t t = 0; t < in.n_queries; ++t) for (uint64_t k = in.cand_off[t]; k < in.cand_off[t + 1]; ++k) W.cq[k] = (uint32_t)t;
        return FDGPU_OK;
    }
    W.wc.reserve(n_wi); W.wi.reserve(n_wi); W.wq.reserve(n_wi); W.wj.reserve(n_wi);
    for (uint64_t t = 0; t < in.n_queries; ++t)
        for (uint64_t k = in.cand_off[t]; k < in.cand_off[t + 1]; ++k) {
            const uint64_t r0 = in.res_off[in.cand[k]], r1 = r0 + len[k];
            for (uint64_t r = r0; r < r1; r += FD_WAVE)
                for (uint64_t j0 = r0; j0 < r1; j0 += j_span ? j_span : len[k]) {
                    W.wc.push_back((uint32_t)k); W.wi.push_back((uint32_t)r); W.wq.push_back((uint32_t)t); W.wj.push_back((uint32_t)j0);
                }
        }
    return FDGPU_OK;
}

// ---- per-query tables ---------------------------------------------------------------------------------------------------
// the query's hashes, its hash set's place (k_mp_qset_build fills it), the residue-type masks and the prefilter rule
static void mp_query_head(const fd_match_query *q, uint32_t hash_type, mp_query_tabs &T, mp_query_dev &Q) {
    Q.qh_off = (uint32_t)T.hashes.size(); Q.n_hashes = (uint32_t)q->n_hashes;
    Q.qs_off = 0; Q.qs_mask = 0;
    if (q->n_hashes > MP_QH_LDS && T.qset_slots + 4 * q->n_hashes < (1ull << 31)) {      // a hash set for the drains' membership test
        uint64_t slots = 2048;
        while (slots < 2 * q->n_hashes) slots <<= 1;
        Q.qs_off = (uint32_t)T.qset_slots; Q.qs_mask = (uint32_t)(slots - 1);
        T.qset_slots += slots; T.qset_max_hashes = std::max<uint64_t>(T.qset_max_hashes, q->n_hashes);
    }
    T.hashes.insert(T.hashes.end(), q->hashes, q->hashes + q->n_hashes);
    Q.aa1_mask = Q.aa2_mask = 0;
    for (uint64_t k = 0; k < q->n_hashes; ++k) {
        uint32_t a1, a2;
        fd_hash_aa_pair(hash_type, q->hashes[k], &a1, &a2);
        Q.aa1_mask |= 1u << (a1 & 31u); Q.aa2_mask |= 1u << (a2 & 31u);
    }
    // TertiaryInteraction (5) / Hybrid (6) hashes carry no residue types: the reference's prefilter unwraps a None there
    // (retrieve.rs:576) and panics for queries of <= 200 hashes; every pair is scanned instead
    const bool no_aa = hash_type == 5u || hash_type == 6u;
    Q.use_prefilter = no_aa ? 0 : q->use_aa_prefilter; Q.ca_window = q->ca_distance_cutoff;
}
static bool mp_typed(const fd_match_query *q, uint64_t e) { return q->aad_aa1[e] < 32 && q->aad_aa2[e] < 32; }      // residue type 255 never passes get_single_feature
static uint32_t mp_group(const fd_match_query *q, uint64_t e) { return q->aad_aa1[e] * 32u + q->aad_aa2[e]; }
// a motif query's dozen observed distances (at most 256): (group << 16 | e) keys sorted (= stable by e), the 1,025-entry start table written as
// a few runs — counting into it and scanning it cost 1,024 dependent adds per query, 128 times per batch
static void mp_group_sorted(const fd_match_query *q, uint32_t *start, mp_query_tabs &T, mp_query_dev &Q) {
    uint32_t keys[256];
    uint32_t nk = 0;
    for (uint64_t e = 0; e < q->n_aad; ++e)
        if (mp_typed(q, e)) keys[nk++] = (mp_group(q, e) << 16) | (uint32_t)e;
    std::sort(keys, keys + nk);
    Q.aad_off = (uint32_t)T.dist.size(); Q.n_aad = nk;
    T.qi.resize(Q.aad_off + nk); T.dist.resize(Q.aad_off + nk);
    uint32_t g_next = 0;       // start[g] for g < g_next is written
    for (uint32_t k = 0; k < nk; ++k) {
        const uint32_t g = keys[k] >> 16, e = keys[k] & 0xffffu;
        if (g >= g_next) { std::fill(start + g_next, start + g + 1, k); g_next = g + 1; }
        T.qi[Q.aad_off + k] = q->aad_qi[e]; T.dist[Q.aad_off + k] = q->aad_dist[e];
    }
    std::fill(start + g_next, start + 1025, nk);
}
// any number of observed distances: counting sort by group (start arrives zeroed)
static void mp_group_counted(const fd_match_query *q, uint32_t *start, mp_query_tabs &T, mp_query_dev &Q) {
    for (uint64_t e = 0; e < q->n_aad; ++e)
        if (mp_typed(q, e)) ++start[mp_group(q, e) + 1];
    for (int k = 0; k < 1024; ++k) start[k + 1] += start[k];
    Q.aad_off = (uint32_t)T.dist.size(); Q.n_aad = start[1024];
    T.qi.resize(Q.aad_off + Q.n_aad); T.dist.resize(Q.aad_off + Q.n_aad);
    uint32_t cur[1024];
    memcpy(cur, start, sizeof cur);
    for (uint64_t e = 0; e < q->n_aad; ++e)
        if (mp_typed(q, e)) {
            const uint32_t k = Q.aad_off + cur[mp_group(q, e)]++;
            T.qi[k] = q->aad_qi[e]; T.dist[k] = q->aad_dist[e];
        }
}
// sorted hash set, residue-type masks, aa_dist_map grouped by (aa_i, aa_j) — stable order inside a group = the observed-list order the reference emits in
void mp_query_tables(const mp_tables_in &in, mp_query_tabs &T) {
    T.qtab.assign(std::max<uint64_t>(in.n_queries, 1), mp_query_dev{});
    T.start.assign((size_t)1025 * in.n_queries, 0u);      // one start table per query, filled in place (a batch of 512 motif queries: 2 MB)
    for (uint64_t t = 0; t < in.n_queries; ++t) {
        const fd_match_query *q = &in.qs[t];
        mp_query_head(q, in.hash_type, T, T.qtab[t]);
        if (q->n_aad <= 256) mp_group_sorted(q, &T.start[(size_t)1025 * t], T, T.qtab[t]);
        else mp_group_counted(q, &T.start[(size_t)1025 * t], T, T.qtab[t]);
        T.want_iv = T.want_iv || T.qtab[t].n_aad > 1024u;
    }
}

// ---- interval tables ----------------------------------------------------------------------------------------------------
// queries whose observed-distance lists do not fit the kernel's LDS copy (whole-structure queries: ~10^2 distances per residue-type
// pair): per group the union of the float intervals {d : |d - x| < window} over its observed x, merged — the scan's window test reads
// one or two intervals instead of walking the list.  Exact: fl(d - x) is monotone in d, so the set of passing d of one x is an interval
// of floats whose ends are found by stepping from x -/+ window to the last float that still passes.
static bool mp_pass_interval(float x, float w, float *lo_out, float *hi_out) {
    if (!(fabsf(x - x) < w)) return false;                  // window <= 0 or NaN: nothing passes
    float hi = x + w, lo = x - w;
    while (!(fabsf(hi - x) < w)) hi = nextafterf(hi, -INFINITY);
    for (float n2 = nextafterf(hi, INFINITY); fabsf(n2 - x) < w; n2 = nextafterf(hi, INFINITY)) hi = n2;
    while (!(fabsf(lo - x) < w)) lo = nextafterf(lo, INFINITY);
    for (float n2 = nextafterf(lo, -INFINITY); fabsf(n2 - x) < w; n2 = nextafterf(lo, -INFINITY)) lo = n2;
    *lo_out = lo; *hi_out = hi;
    return true;
}
// one group's observed distances x[0 .. n) -> its intervals appended to out, ascending; neighbours with no float between them are one interval
static void mp_merge_group(const float *x, uint32_t n, float w, std::vector<std::pair<float, float>> &tmp, std::vector<float> &out) {
    tmp.clear();
    for (uint32_t e = 0; e < n; ++e) {
        float lo, hi;
        if (mp_pass_interval(x[e], w, &lo, &hi)) tmp.emplace_back(lo, hi);
    }
    std::sort(tmp.begin(), tmp.end());
    for (size_t k = 0; k < tmp.size();) {
        float lo = tmp[k].first, hi = tmp[k].second;
        size_t z = k + 1;
        while (z < tmp.size() && tmp[z].first <= nextafterf(hi, INFINITY)) { hi = std::max(hi, tmp[z].second); ++z; }
        out.push_back(lo); out.push_back(hi);
        k = z;
    }
}
// one query: V.iv_start[1025 * t ..] and its intervals appended to V.lohi.  The 1,024 groups are independent: eight parts of 128 groups on the helper
// threads when the query observes enough distances to pay for waking them (a whole-structure query: ~3·10^4 observed distances, six nextafterf each),
// stitched in group order afterwards
static void mp_query_intervals(const uint32_t *stt, const float *base, float w, fd_host_pool *pool, uint32_t *iv_start, std::vector<float> &lohi) {
    constexpr unsigned NP = 8;
    std::vector<float> part_lohi[NP];
    uint32_t g_cnt[1024];
    auto groups = [&](unsigned part) {
        std::vector<std::pair<float, float>> tmp;
        for (int g = 128 * (int)part; g < 128 * ((int)part + 1); ++g) {
            const size_t before = part_lohi[part].size();
            mp_merge_group(base + stt[g], stt[g + 1] - stt[g], w, tmp, part_lohi[part]);
            g_cnt[g] = (uint32_t)((part_lohi[part].size() - before) / 2);
        }
    };
    if (!pool || stt[1024] - stt[0] < 8192u) { for (unsigned k = 0; k < NP; ++k) groups(k); }
    else {
        std::atomic<unsigned> next_part(0);
        const std::function<void()> wk = [&]() { for (;;) { const unsigned k = next_part.fetch_add(1); if (k >= NP) break; groups(k); } };
        pool->run(std::min(NP, std::max(1u, std::thread::hardware_concurrency())), wk);
    }
    uint32_t run = (uint32_t)(lohi.size() / 2);
    for (unsigned k = 0; k < NP; ++k) lohi.insert(lohi.end(), part_lohi[k].begin(), part_lohi[k].end());      // the parts in group order
    for (int g = 0; g < 1024; ++g) { iv_start[g] = run; run += g_cnt[g]; }
    iv_start[1024] = run;
}
void mp_interval_tables(uint64_t n_queries, const mp_query_tabs &T, fd_host_pool *pool, mp_intervals &V) {
    V.iv_start.assign((size_t)1025 * n_queries, 0);
    for (uint64_t t = 0; t < n_queries; ++t)
        mp_query_intervals(&T.start[1025 * t], T.dist.data() + T.qtab[t].aad_off, T.qtab[t].ca_window, pool, &V.iv_start[1025 * t], V.lohi);
}

// ---- layout and packing -------------------------------------------------------------------------------------------------
// one packed host block -> one H2D copy: [cand | wc | wi | wq | wj | hashes | start tables | dist | qi | qtab | iv_start | iv | iv_grp | wbase | cq]
mp_layout mp_make_layout(uint64_t n_cand, uint64_t n_queries, bool dev_items, const mp_built &B) {
    const size_t nw = dev_items ? B.W.n_wi : B.W.wc.size(), na = B.T.dist.size();
    const bool iv = B.T.want_iv;
    mp_layout L;
    L.cand = 0; L.wc = L.cand + mp_up4(n_cand); L.wi = L.wc + mp_up4(nw); L.wq = L.wi + mp_up4(nw); L.wj = L.wq + mp_up4(nw);
    L.hashes = L.wj + mp_up4(nw); L.start = L.hashes + mp_up4(B.T.hashes.size()); L.dist = L.start + mp_up4(B.T.start.size());
    L.qi = L.dist + mp_up4(na); L.qtab = L.qi + mp_up4(na); L.iv_start = L.qtab + mp_up4(n_queries * (sizeof(mp_query_dev) / 4));
    L.iv = L.iv_start + (iv ? mp_up4(B.V.iv_start.size()) : 0); L.iv_grp = L.iv + (iv ? mp_up4(B.V.lohi.size()) : 0);
    L.wbase = L.iv_grp + (iv ? 1024 * n_queries : 0); L.cq = L.wbase + (dev_items ? mp_up4(n_cand + 1) : 0);
    L.words = L.cq + (dev_items ? mp_up4(n_cand) : 0) + 4;
    return L;
}
static void mp_put(uint32_t *blk, size_t at, const void *src, size_t n_words) { if (n_words) memcpy(blk + at, src, n_words * 4); }
void mp_pack(const mp_tables_in &in, const mp_layout &L, const mp_built &B, uint32_t *blk) {
    const uint64_t n_cand = in.cand_off[in.n_queries], n_queries = in.n_queries;
    mp_put(blk, L.cand, in.cand, n_cand);
    if (in.dev_items) { mp_put(blk, L.wbase, B.W.wbase.data(), n_cand + 1); mp_put(blk, L.cq, B.W.cq.data(), n_cand); }
    else {
        const size_t nw = B.W.wc.size();
        mp_put(blk, L.wc, B.W.wc.data(), nw); mp_put(blk, L.wi, B.W.wi.data(), nw); mp_put(blk, L.wq, B.W.wq.data(), nw); mp_put(blk, L.wj, B.W.wj.data(), nw);
    }
    mp_put(blk, L.hashes, B.T.hashes.data(), B.T.hashes.size());
    mp_put(blk, L.start, B.T.start.data(), B.T.start.size());
    mp_put(blk, L.dist, B.T.dist.data(), B.T.dist.size()); mp_put(blk, L.qi, B.T.qi.data(), B.T.qi.size());
    mp_put(blk, L.qtab, B.T.qtab.data(), n_queries * (sizeof(mp_query_dev) / 4));
    if (!B.T.want_iv) return;
    mp_put(blk, L.iv_start, B.V.iv_start.data(), B.V.iv_start.size());
    mp_put(blk, L.iv, B.V.lohi.data(), B.V.lohi.size());
    // the scan's LDS copy: per query and group (first interval relative to the query's first) << 8 | number of intervals (a window of 1 A
    // leaves 1-5 disjoint intervals per group of a 300-residue query, ~700 in all; 255+ intervals of one group: the count saturates and
    // the scan walks that group in global memory)
    for (uint64_t t = 0; t < n_queries; ++t)
        for (int g = 0; g < 1024; ++g) {
            const uint32_t v_lo = B.V.iv_start[1025 * t + g], v_hi = B.V.iv_start[1025 * t + g + 1], rel = v_lo - B.V.iv_start[1025 * t];
            blk[L.iv_grp + 1024 * t + g] = (std::min<uint32_t>(rel, 0xffffffu) << 8) | std::min<uint32_t>(v_hi - v_lo, 255u);
        }
}

int mp_build_tables(const mp_tables_in &in, fd_host_pool *pool, mp_built &B, fd_mp_tables &TB, const char **err) {
    const int rc = mp_work_items(in, B.W, err);
    if (rc) return rc;
    mp_query_tables(in, B.T);
    if (B.T.want_iv) mp_interval_tables(in.n_queries, B.T, pool, B.V);
    TB.L = mp_make_layout(in.cand_off[in.n_queries], in.n_queries, in.dev_items, B);
    TB.nw = in.dev_items ? B.W.n_wi : B.W.wc.size(); TB.j_span = B.W.j_span; TB.want_iv = B.T.want_iv; TB.dev_items = in.dev_items;
    TB.qset_slots = B.T.qset_slots; TB.qset_max_hashes = B.T.qset_max_hashes;
    return FDGPU_OK;
}

// ---- test-only entry (include/fdgpu_debug.h) -----------------------------------------------------------------------------
extern "C" int fdgpu_debug_match_tables(uint64_t n_queries, const fd_match_query *qs, const uint32_t *cand, const uint64_t *cand_off, const uint64_t *res_off,
                                        uint64_t n_struct, uint32_t hash_type, uint32_t dev_items, uint32_t pooled, uint32_t **block, uint64_t *layout,
                                        uint64_t *scalars, const char **message) {
    if (!cand_off || !res_off || !block || !layout || !scalars || !message || (n_queries && !qs) || (cand_off[n_queries] && !cand)) return FDGPU_EINVAL;
    *block = nullptr; *message = nullptr;
    const mp_tables_in in = {n_queries, qs, cand, cand_off, res_off, n_struct, hash_type, dev_items != 0};
    fd_host_pool pool;
    mp_built B;
    fd_mp_tables TB;
    const int rc = mp_build_tables(in, pooled ? &pool : nullptr, B, TB, message);
    if (rc) return rc;
    const mp_layout &L = TB.L;
    const size_t offs[16] = {L.cand, L.wc, L.wi, L.wq, L.wj, L.hashes, L.start, L.dist, L.qi, L.qtab, L.iv_start, L.iv, L.iv_grp, L.wbase, L.cq, L.words};
    for (int k = 0; k < 16; ++k) layout[k] = offs[k];
    scalars[0] = TB.nw; scalars[1] = TB.j_span; scalars[2] = TB.want_iv ? 1 : 0; scalars[3] = TB.qset_slots; scalars[4] = TB.qset_max_hashes;
    uint32_t *blk = (uint32_t *)calloc(L.words, 4);
    if (!blk) return FDGPU_ENOMEM;
    mp_pack(in, L, B, blk);
    *block = blk;
    return FDGPU_OK;
}
