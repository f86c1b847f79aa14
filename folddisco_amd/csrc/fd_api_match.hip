// fd_api_match.hip — C ABI of libfdgpu.so, seam S4 (include/fdgpu.h): the pair scan over candidates, superposition, metrics and LMS-QCP — the
// orchestration of k_match.hip.  Reference: src/controller/retrieve.rs:52-156, src/structure/kabsch.rs:157-554, src/structure/metrics.rs:62-251,
// src/structure/lms_qcp.rs.
// The pair scan (fd_match_pairs_multi) is a sequence of stages: mp_choose_form -> mp_host_tables (fd_match_tables.cpp) -> mp_upload_tables ->
// mp_upload_votes -> mp_fill_args -> mp_scan (mp_reserve_queue per attempt) -> one way out: mp_vote_rows, mp_out_on_device, mp_out_packed, mp_out_records.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <atomic>
#include <memory>
#include <thread>
#include "fdgpu_internal.h"
#include "fd_api_common.h"

// found triples in the reference's scan order — (slot, i, j), several bin pairs of one (i, j) in emission order — from the kernel's
// append order: counting sort by slot (stable), then the slots' runs sorted independently on host threads (a whole-structure query
// returns ~10^5 triples for a handful of slots: one 20 ms std::stable_sort otherwise)
static void fd_sort_found(fd_pair_rec *f, uint64_t n, uint64_t n_cand) {
    if (n < 2) return;
    auto by_ij = [](const fd_pair_rec &a, const fd_pair_rec &b) { return a.i != b.i ? a.i < b.i : a.j < b.j; };
    if (n < 4096 || n_cand == 0) {
        std::stable_sort(f, f + n, [&](const fd_pair_rec &a, const fd_pair_rec &b) { return a.cand != b.cand ? a.cand < b.cand : by_ij(a, b); });
        return;
    }
    std::vector<uint64_t> start(n_cand + 2, 0);
    for (uint64_t k = 0; k < n; ++k) ++start[std::min<uint64_t>(f[k].cand, n_cand) + 1];
    for (uint64_t s = 0; s <= n_cand; ++s) start[s + 1] += start[s];
    std::vector<fd_pair_rec> tmp(n);
    {
        std::vector<uint64_t> cur(start.begin(), start.end() - 1);
        for (uint64_t k = 0; k < n; ++k) tmp[cur[std::min<uint64_t>(f[k].cand, n_cand)]++] = f[k];
    }
    std::atomic<uint64_t> next(0);
    auto work = [&]() {
        for (;;) {
            const uint64_t s = next.fetch_add(1);
            if (s > n_cand) break;
            std::stable_sort(tmp.begin() + start[s], tmp.begin() + start[s + 1], by_ij);
        }
    };
    const unsigned T = (unsigned)std::min<uint64_t>(std::min<uint64_t>(16, std::max(1u, std::thread::hardware_concurrency())), n_cand + 1);
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    memcpy(f, tmp.data(), n * sizeof(fd_pair_rec));
}

// FDGPU_TRACE: a call's clock, and its lines "[tag] what at <ms since the call began> ms<detail>" on stderr
struct fd_call_trace {
    bool on = false;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    static fd_call_trace from_env() { fd_call_trace t; t.on = getenv("FDGPU_TRACE") != nullptr; return t; }
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    void line(const char *tag, const char *what) const { line(tag, what, "%s", ""); }
    __attribute__((format(printf, 4, 5))) void line(const char *tag, const char *what, const char *detail_fmt, ...) const {
        if (!on) return;
        char detail[256];
        va_list ap;
        va_start(ap, detail_fmt);
        vsnprintf(detail, sizeof detail, detail_fmt, ap);
        va_end(ap);
        fprintf(stderr, "[%s] %s at %.3f ms%s\n", tag, what, ms(), detail);
    }
};

// ---- S4 ---------------------------------------------------------------------------------------------------------------
namespace {
// a pair scan's arguments as every stage reads them (n_cand: set by mp_choose_form once cand_off is known to be there)
struct mp_in {
    fdgpu_ctx *c; const fdgpu_batch *db; const uint8_t *resname_std; uint64_t n_queries; const fd_match_query *qs; const uint32_t *cand; const uint64_t *cand_off;
    const fd_hash_params *p; const fd_mp_request &rq; uint64_t n_cand;
};
struct mp_out { fd_pair_rec **found; uint64_t *n_found; fd_cand_rec **cands; uint64_t *n_cands; };
// what the environment decides, read once
struct mp_form {
    fd_call_trace tr;
    bool dev_items = false;                 // the work items are written on the device (one-off blocks); FDGPU_MP_ITEMS=0: host-built items (tests)
    uint64_t pack_min = 1ull << 18;         // candidate pairs from which the packed form pays (a motif query's few thousand pairs are cheaper as they are); FDGPU_PACK_MIN (tests)
    uint64_t found_sort_min = 32768;        // found triples from which the device sorts them; FDGPU_FOUND_SORT=device: 2, =host: never (tests)
    bool found_sort_host = false;
};
struct mp_totals { uint64_t found = 0, cands = 0; };
// byte offsets of the rescue vote tables in ws[WS_IDS_B] (MP_VOTES): per slot vt_off / vt_qs, per row its first counter, the row itself (written by
// k_vote_rows) and its length, per marked partner residue its component, the sorted observed-distance lists
struct mp_vote_layout { uint64_t off = 0, roff = 0, rows = 0, qs = 0, rlen = 0, comp = 0, sdd = 0, sdq = 0, bytes = 0; };
struct mp_free { void operator()(void *p) const { free(p); } };
template <typename T> using mp_host = std::unique_ptr<T, mp_free>;      // host results on their way out: the caller's (libc free) once released
template <typename T> mp_host<T> mp_host_alloc(uint64_t n) { return mp_host<T>((T *)malloc(std::max<uint64_t>(n, 1) * sizeof(T))); }
}  // namespace

// Every refusal of the call, and what the environment switches choose.  The legal modes: MP_VOTES alone, with a vote plan and the partner mask;
// else any of MP_FOUND / MP_CANDS, with MP_ON_DEVICE (nothing else then), or MP_CANDS_UNORDERED / MP_CANDS_PACKED beside MP_CANDS.
static int mp_choose_form(mp_in &I, const mp_out &O, mp_form &F) {
    fdgpu_ctx *c = I.c;
    const fd_mp_request &rq = I.rq;
    if (!c || !I.db || !I.p || !O.found || !O.n_found || !O.cands || !O.n_cands || !I.cand_off || (I.n_queries && !I.qs)) return FDGPU_EINVAL;
    const uint32_t mode = rq.mode;
    if (mode & MP_VOTES) { if (mode != MP_VOTES || !rq.votes || !rq.cj_mask || !rq.mask_off) return FDGPU_EINVAL; }
    else if (mode & MP_ON_DEVICE) { if (mode & ~(MP_ON_DEVICE | MP_FOUND | MP_CANDS)) return FDGPU_EINVAL; }
    else if ((mode & ~(MP_FOUND | MP_CANDS | MP_CANDS_UNORDERED | MP_CANDS_PACKED)) || ((mode & (MP_CANDS_UNORDERED | MP_CANDS_PACKED)) && !(mode & MP_CANDS))) return FDGPU_EINVAL;
    I.n_cand = I.cand_off[I.n_queries];
    if (I.n_cand && !I.cand) return FDGPU_EINVAL;
    *O.found = nullptr; *O.cands = nullptr; *O.n_found = 0; *O.n_cands = 0;
    if (!fd_hash_type_supported(I.p->hash_type)) FAIL(c, FDGPU_EINVAL, "hash_type: only the encodings over the (d_CA, d_CB, theta, tau1, tau2) descriptor are built (0, 1, 3, 7, 8)");
    reset_timings(c);
    F.tr = fd_call_trace::from_env();
    if (!fd_multiple_bins_valid(I.p)) FAIL(c, FDGPU_EINVAL, "multiple_bins: at most 8 (dist, angle) bin pairs, no zero counts");
    const char *it_env = getenv("FDGPU_MP_ITEMS"), *pm_env = getenv("FDGPU_PACK_MIN"), *fs_env = getenv("FDGPU_FOUND_SORT");
    F.dev_items = !rq.tables && I.n_cand < (1ull << 24) && !(it_env && it_env[0] == '0');
    if (pm_env) F.pack_min = strtoull(pm_env, nullptr, 10);
    if (fs_env && !strcmp(fs_env, "device")) F.found_sort_min = 2;
    F.found_sort_host = fs_env && !strcmp(fs_env, "host");
    return FDGPU_OK;
}

// Work items and query tables depend on the queries and candidates only: a caller that scans the same candidates twice (the two scans of a large query)
// passes a fd_mp_tables and the second call reuses the host block.  A caller that keeps the tables gets them in a vector; a one-off block (a batch of
// motif queries: ~3.5 MB per 512 queries) is packed straight into the context's pinned staging buffer — its copy is then a DMA, not a staged pageable copy
static int mp_host_tables(const mp_in &I, const mp_form &F, fd_mp_tables &TB) {
    fdgpu_ctx *c = I.c;
    const mp_tables_in in = {I.n_queries, I.qs, I.cand, I.cand_off, I.db->h_res_off.data(), I.db->n_struct, I.p->hash_type, F.dev_items};
    mp_built B;
    const char *msg = nullptr;
    const int rc = mp_build_tables(in, c->is_lane ? nullptr : &c->host_pool, B, TB, &msg);      // (a lane's short host loops stay on its own thread)
    if (rc) FAIL(c, rc, msg);
    uint32_t *blk = I.rq.tables ? nullptr : (uint32_t *)c->host_pinned(FD_HP_SCAN_A, TB.L.words * 4);
    if (!blk) { TB.blk.assign(TB.L.words, 0); blk = TB.blk.data(); }
    mp_pack(in, TB.L, B, blk);
    TB.data = blk; TB.valid = true;
    return FDGPU_OK;
}

// the block -> ws[WS_MISC0] (device-written items: without the item arrays, which k_mp_items writes — and, per candidate, the list of its active
// residues), resname_std -> ws[WS_MISC5], the partner-residue filter (second pass of a large query's retrieval) -> ws[WS_MISC1]
static int mp_upload_tables(const mp_in &I, const fd_mp_tables &TB, mp_args &A) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    const fdgpu_batch *db = I.db;
    const mp_layout &L = TB.L;
    const uint64_t n_cand = I.n_cand;
    HIPCHK(c, c->ws[WS_MISC0].ensure(L.words * 4));
    if (I.resname_std) {
        HIPCHK(c, c->ws[WS_MISC5].ensure(std::max<uint64_t>(db->n_res, 1)));
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC5].p, I.resname_std, db->n_res, hipMemcpyHostToDevice, st));
        A.resname_std = c->ws[WS_MISC5].as<uint8_t>();
    }
    uint32_t *d = c->ws[WS_MISC0].as<uint32_t>();
    if (TB.dev_items) {
        HIPCHK(c, hipMemcpyAsync(d, TB.data, L.wc * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d + L.hashes, TB.data + L.hashes, (L.words - L.hashes) * 4, hipMemcpyHostToDevice, st));
        const size_t ci_bytes = ((size_t)n_cand * 16 + 255) & ~(size_t)255;
        HIPCHK(c, c->ws[WS_MP_ACT].ensure(ci_bytes + (size_t)64 * std::max<size_t>(TB.nw, 1) * 4));
        A.cinfo = c->ws[WS_MP_ACT].as<uint4>();
        A.act = (const uint32_t *)(c->ws[WS_MP_ACT].as<uint8_t>() + ci_bytes);
        fd_launch_mp_items(db->res_off, d + L.cand, (uint32_t)n_cand, d + L.wbase, d + L.cq, TB.j_span, d + L.wc, d + L.wi, d + L.wq, d + L.wj, st, db->aa, db->hash_ok,
                           A.resname_std, fd_make_consts_cfg(I.p, 0).q.type == FD_HASH_TERTIARY ? 1 : 0, (const mp_query_dev *)(d + L.qtab), (void *)A.cinfo, (uint32_t *)A.act);
    } else
        HIPCHK(c, hipMemcpyAsync(d, TB.data, L.words * 4, hipMemcpyHostToDevice, st));
    if (I.rq.cj_mask && I.rq.mask_off) {
        const uint64_t mask_words = I.rq.mask_words;
        HIPCHK(c, c->ws[WS_MISC1].ensure((mask_words + n_cand + 2) * 4));
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC1].p, I.rq.cj_mask, mask_words * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC1].as<uint32_t>() + mask_words, I.rq.mask_off, n_cand * 4, hipMemcpyHostToDevice, st));
        A.cj_mask = c->ws[WS_MISC1].as<uint32_t>(); A.mask_off = A.cj_mask + mask_words;
    }
    return FDGPU_OK;
}

static mp_vote_layout mp_make_vote_layout(uint64_t n_cand, const fd_vote_plan &v) {
    auto up8 = [](uint64_t x) { return (x + 7) & ~(uint64_t)7; };
    mp_vote_layout V;
    V.off = 0; V.roff = V.off + up8(n_cand * 8); V.rows = V.roff + up8(v.n_rows * 8); V.qs = V.rows + up8(v.n_rows * sizeof(fd_vote_row));
    V.rlen = V.qs + up8(n_cand * 4); V.comp = V.rlen + up8(v.n_rows * 4); V.sdd = V.comp + up8(v.n_bits); V.sdq = V.sdd + up8(v.n_sd * 4);
    V.bytes = V.sdq + up8(v.n_sd * 4) + 8;
    return V;
}
// MP_VOTES, the rescue votes stay on the device: counters in ws[WS_IDS_A] (zeroed), their tables in ws[WS_IDS_B]
static int mp_upload_votes(const mp_in &I, mp_vote_layout &V, mp_args &A) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    const fd_vote_plan *votes = I.rq.votes;
    const uint64_t n_cand = I.n_cand, nb = votes->n_bits, nr = votes->n_rows;
    V = mp_make_vote_layout(n_cand, *votes);
    HIPCHK(c, c->ws[WS_IDS_A].ensure(std::max<uint64_t>(votes->n_counters, 1) * 4));
    HIPCHK(c, c->ws[WS_IDS_B].ensure(V.bytes));
    uint8_t *base = c->ws[WS_IDS_B].as<uint8_t>();
    HIPCHK(c, hipMemsetAsync(c->ws[WS_IDS_A].p, 0, std::max<uint64_t>(votes->n_counters, 1) * 4, st));
    HIPCHK(c, hipMemcpyAsync(base + V.off, votes->vt_off, n_cand * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(base + V.qs, votes->vt_qs, n_cand * 4, hipMemcpyHostToDevice, st));
    if (nr) {
        HIPCHK(c, hipMemcpyAsync(base + V.roff, votes->row_off, nr * 8, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(base + V.rlen, votes->row_len, nr * 4, hipMemcpyHostToDevice, st));
    }
    if (nb) HIPCHK(c, hipMemcpyAsync(base + V.comp, votes->cj_comp, nb, hipMemcpyHostToDevice, st));
    A.votes = c->ws[WS_IDS_A].as<uint32_t>(); A.vt_off = (const uint64_t *)(base + V.off); A.vt_qs = (const uint32_t *)(base + V.qs);
    A.cj_comp = base + V.comp;
    if (votes->sd_dist && votes->sd_qi && votes->n_sd) {
        HIPCHK(c, hipMemcpyAsync(base + V.sdd, votes->sd_dist, votes->n_sd * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(base + V.sdq, votes->sd_qi, votes->n_sd * 4, hipMemcpyHostToDevice, st));
        A.sd_dist = (const float *)(base + V.sdd); A.sd_qi = (const uint32_t *)(base + V.sdq);
    }
    return FDGPU_OK;
}

// the kernels' arguments from the block's layout; the hash sets of queries that hold more hashes than a drain stages in LDS; the counters
static int mp_fill_args(const mp_in &I, const fd_mp_tables &TB, mp_args &A) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    const fd_hash_params *p = I.p;
    const mp_layout &L = TB.L;
    const uint32_t *dblk = c->ws[WS_MISC0].as<uint32_t>();
    const bool want_iv = TB.want_iv;      // some query observes more than 1,024 distances
    A.B = I.db->view(); A.C = fd_make_consts_cfg(p, 0); A.cutoff = p->dist_cutoff;
    A.n_cfg = fd_num_bin_configs(p);
    for (uint32_t k = 0; k < A.n_cfg; ++k) A.qk[k] = fd_make_consts_cfg(p, k).q;
    A.cand = dblk + L.cand; A.n_cand = (uint32_t)I.n_cand;
    A.wi_cand = dblk + L.wc; A.wi_i0 = dblk + L.wi; A.wi_query = dblk + L.wq; A.n_work = (uint32_t)TB.nw;
    A.wi_j0 = dblk + L.wj; A.j_span = TB.j_span;
    A.q_hashes = dblk + L.hashes; A.aad_start = dblk + L.start; A.aad_dist = (const float *)(dblk + L.dist); A.aad_qi = dblk + L.qi;
    A.iv_start = want_iv ? dblk + L.iv_start : nullptr; A.iv = want_iv ? (const float2 *)(dblk + L.iv) : nullptr;
    A.iv_grp = want_iv ? dblk + L.iv_grp : nullptr;
    A.qtab = (const mp_query_dev *)(dblk + L.qtab);
    A.compact = !want_iv;
    if ((I.rq.mode & MP_FOUND) && TB.qset_slots) {
        HIPCHK(c, c->ws[WS_MP_QSET].ensure(TB.qset_slots * 4));
        HIPCHK(c, hipMemsetAsync(c->ws[WS_MP_QSET].p, 0xff, TB.qset_slots * 4, st));
        fd_launch_mp_qset_build(A.qtab, (uint32_t)I.n_queries, (uint32_t)TB.qset_max_hashes, dblk + L.hashes, c->ws[WS_MP_QSET].as<uint32_t>(), st);
        A.qset = c->ws[WS_MP_QSET].as<uint32_t>();
    }
    // ws[WS_TOTAL] (u64): [0] found triples, [1] candidate pairs, [2] chunks drained, from [16]: the 64 sub-queues' claimed chunks, one per 128-byte line
    HIPCHK(c, c->ws[WS_TOTAL].ensure(16384));
    A.n_found = c->ws[WS_TOTAL].as<unsigned long long>(); A.n_cands = A.n_found + 1; A.q_cnt = A.n_found + 16;
    return FDGPU_OK;
}

// the chunk queue between the scan and the drains for one attempt (q_max: most chunks one sub-queue was asked for by the attempt before), and on a new
// allocation the drains' bin tables, once
static int mp_reserve_queue(const mp_in &I, size_t nw, uint64_t q_max, mp_args &A) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    // the chunk queue between the scan and the drains, ws[WS_MP_Q]: [256 B bin tables | per chunk: 16 B header, 256 B pairs, 3 x 256 B results,
    // 8 B totals, 16 B positions], 64 sub-queues.  A work item rarely queues more than two chunks; a launch that asks for more than a sub-queue
    // holds counts them and is repeated with the queue it asked for
    const uint64_t per = 16 + 256 + 768 + 8 + 16, have = c->ws[WS_MP_Q].cap > 256 ? (c->ws[WS_MP_Q].cap - 256) / (per * 64) : 0;
    uint64_t want = std::max<uint64_t>(have, std::max<uint64_t>(64, (nw + nw / 2) / 64 + 32));
    if (q_max > have) want = std::max<uint64_t>(want, q_max + q_max / 4 + 16);
    if (want > have) HIPCHK(c, c->ws[WS_MP_Q].ensure(256 + want * per * 64));
    if (c->ws[WS_MP_Q].p != c->mp_bintab_at || c->ws[WS_MP_Q].cap != c->mp_bintab_cap) {      // (a new allocation: the tables once)
        uint32_t t64[64];
        memset(t64, 0, sizeof t64);
        fd_fill_bintab(t64);
        for (int k = 0; k < FD_BINTAB_WORDS; ++k) t64[32 + k] = t64[k];
        for (int m = 0; m < 4; ++m)
            for (int k = 0; k < 4; ++k) { const uint32_t v = t64[32 + 7 + 5 * m + k]; t64[32 + 7 + 5 * m + k] = v > 0x7f7fffffu ? 0x7f7fffffu : v; }
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_MP_Q].p, t64, sizeof t64, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->mp_bintab_at = c->ws[WS_MP_Q].p; c->mp_bintab_cap = c->ws[WS_MP_Q].cap;
    }
    const uint64_t capq = std::min<uint64_t>((c->ws[WS_MP_Q].cap - 256) / (per * 64), 0x1ffffffu), nch = capq * 64;
    uint8_t *qb = c->ws[WS_MP_Q].as<uint8_t>() + 256;
    A.cap_subq = (uint32_t)capq;
    A.bintab = c->ws[WS_MP_Q].as<uint32_t>();
    A.chunk_base = (ulonglong2 *)qb; qb += nch * 16;
    A.chunk_hdr = (uint4 *)qb; qb += nch * 16;
    A.chunk_cnt = (uint2 *)qb; qb += nch * 8;
    A.chunk_ij = (uint32_t *)qb; qb += nch * 256;
    A.res_h = (uint32_t *)qb; qb += nch * 256;
    A.res_meta = (uint32_t *)qb; qb += nch * 256;
    A.res_d = (float *)qb;
    return FDGPU_OK;
}

// one emitting pass into buffers sized by the previous calls; a pass that overflows only counts, the buffers grow and
// the pass is repeated (the scan is deterministic up to record order, which the ways out restore)
static int mp_scan(const mp_in &I, size_t nw, mp_args &A, mp_totals &T) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    const uint32_t mode = I.rq.mode;
    const fd_vote_plan *votes = I.rq.votes;
    const std::function<void()> *while_scanning = I.rq.while_scanning;
    static_assert(MP_SUBQ_STRIDE == 16, "ws[WS_TOTAL] layout");
    std::vector<uint64_t> tot_v(16 + 64 * MP_SUBQ_STRIDE, 0);
    uint64_t *tot = tot_v.data();
    uint64_t q_max = 0;      // most chunks one sub-queue was asked for by the previous attempt
    for (int attempt = 0; attempt < 4; ++attempt) {
        uint64_t capf = c->ws[WS_KEYS_A].cap / sizeof(fd_pair_rec), capc = c->ws[WS_KEYS_B].cap / sizeof(fd_cand_rec);
        if (capf < 4096 || capf < tot[0]) { HIPCHK(c, c->ws[WS_KEYS_A].ensure(std::max<uint64_t>(2 * tot[0], 65536) * sizeof(fd_pair_rec))); }
        if (capc < 4096 || capc < tot[1]) { HIPCHK(c, c->ws[WS_KEYS_B].ensure(std::max<uint64_t>(2 * tot[1], 65536) * sizeof(fd_cand_rec))); }
        A.found = c->ws[WS_KEYS_A].as<fd_pair_rec>(); A.cands = c->ws[WS_KEYS_B].as<fd_cand_rec>();
        A.cap_found = c->ws[WS_KEYS_A].cap / sizeof(fd_pair_rec); A.cap_cands = c->ws[WS_KEYS_B].cap / sizeof(fd_cand_rec);
        const int rcq = mp_reserve_queue(I, nw, q_max, A);
        if (rcq) return rcq;
        HIPCHK(c, hipMemsetAsync(c->ws[WS_TOTAL].p, 0, tot_v.size() * 8, st));
        // a repeated launch drains its chunks again: the rescue votes of the attempt before (atomic adds of the chunks that did fit) must not count twice
        if (attempt && (mode & MP_VOTES)) HIPCHK(c, hipMemsetAsync(c->ws[WS_IDS_A].p, 0, std::max<uint64_t>(votes->n_counters, 1) * 4, st));
        {
            StageTimer t(c, "match_pairs", 0);
            fd_launch_match_pairs(A, st);
        }
        HIPCHK(c, hipGetLastError());
        if (attempt == 0 && while_scanning && *while_scanning) (*while_scanning)();      // before the copy: one into pageable memory waits for the stream
        HIPCHK(c, hipMemcpyAsync(tot, c->ws[WS_TOTAL].p, tot_v.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        q_max = 0;
        for (int k = 0; k < 64; ++k) q_max = std::max<uint64_t>(q_max, tot[16 + MP_SUBQ_STRIDE * k]);
        if (q_max > A.cap_subq) {      // the drains saw a part of the pairs only: their counts mean nothing
            if (attempt == 3) FAIL(c, FDGPU_ERANGE, "match_pairs: the pair queue did not fit after regrowing");
            tot[0] = tot[1] = 0;
            continue;
        }
        if (tot[0] <= A.cap_found && tot[1] <= A.cap_cands) break;
        if (attempt == 3) FAIL(c, FDGPU_ERANGE, "match_pairs: output did not fit after regrowing");
    }
    T.found = tot[0]; T.cands = tot[1];
    return FDGPU_OK;
}

// MP_VOTES: the rows of the vote table — (largest count, how many hold it, which) per (slot, component, query residue) — to the caller's plan
static int mp_vote_rows(const mp_in &I, const mp_form &F, const mp_vote_layout &V, const mp_args &A) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    const fd_vote_plan *votes = I.rq.votes;
    const uint8_t *base = c->ws[WS_IDS_B].as<uint8_t>();
    const uint64_t nr = votes->n_rows;
    fd_vote_row *d_rows = (fd_vote_row *)(base + V.rows);
    fd_launch_vote_rows(A.votes, (const uint64_t *)(base + V.roff), (const uint32_t *)(base + V.rlen), nr, d_rows, st);
    HIPCHK(c, hipGetLastError());
    if (nr) HIPCHK(c, hipMemcpyAsync(votes->rows, d_rows, nr * sizeof(fd_vote_row), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    F.tr.line("match_pairs", "vote rows done", " (%llu rows, %llu counters)", (unsigned long long)nr, (unsigned long long)votes->n_counters);
    return FDGPU_OK;
}

// MP_ON_DEVICE: the records stay on the device (ws[WS_KEYS_A] = found triples, ws[WS_KEYS_B] = candidate pairs, in append order) for
// the device-side retrieval glue (k_retrieve.hip); only the counts return
static int mp_out_on_device(const mp_totals &T, const mp_out &O) {
    *O.n_found = T.found; *O.n_cands = T.cands;
    return FDGPU_OK;
}

// the stable pair sort's scratch for n pairs (sort_pairs): keys and values twice in ws[WS_MISC2 .. 5], tile histograms, totals
static int mp_sort_scratch(fdgpu_ctx *c, uint64_t n) {
    HIPCHK(c, c->ws[WS_MISC2].ensure(n * 4)); HIPCHK(c, c->ws[WS_MISC3].ensure(n * 4));
    HIPCHK(c, c->ws[WS_MISC4].ensure(n * 4)); HIPCHK(c, c->ws[WS_MISC5].ensure(n * 4));
    HIPCHK(c, c->ws[WS_GHIST].ensure((size_t)256 * std::max<uint32_t>(fd_rs_num_tiles(n), 1) * 4));
    HIPCHK(c, c->ws[WS_TOT].ensure((256 + (size_t)(fd_rs_num_tiles(n) / 128 + 2) * 256) * 8));
    return FDGPU_OK;
}

// MP_CANDS_PACKED (with pk_key / pk_val): the candidate pairs come back packed — key = slot << 16 | partner residue j, value =
// query residue << 16 | residue i — and sorted by key on the device: half the bytes over PCIe and no bucketing on the host
// (the rescue walks the pairs of one partner residue at a time).  Needs slots, residues and query residues below 2^16.
static bool mp_packs(const mp_in &I, const mp_form &F, const mp_totals &T) {
    return (I.rq.mode & MP_CANDS_PACKED) && I.rq.pk_key && I.rq.pk_val && I.n_cand < 65536 && T.cands >= F.pack_min;
}
static int mp_out_packed(const mp_in &I, const mp_form &F, const mp_args &A, const mp_totals &T, const mp_out &O) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    const uint64_t n = T.cands;
    // the packed pairs land in pinned buffers the CONTEXT keeps (valid until the next packed scan on this context; never freed by the caller)
    uint32_t *hk = (uint32_t *)c->host_pinned(FD_HP_SCAN_A, std::max<uint64_t>(n, 1) * 4), *hv = (uint32_t *)c->host_pinned(FD_HP_SCAN_B, std::max<uint64_t>(n, 1) * 4);
    mp_host<fd_pair_rec> hf = mp_host_alloc<fd_pair_rec>(T.found);
    if (!hk || !hv || !hf) return FDGPU_ENOMEM;
    if (n) {
        const int rcs = mp_sort_scratch(c, n);
        if (rcs) return rcs;
        uint32_t *ka = c->ws[WS_MISC2].as<uint32_t>(), *va = c->ws[WS_MISC3].as<uint32_t>(), *kb = c->ws[WS_MISC4].as<uint32_t>(), *vb = c->ws[WS_MISC5].as<uint32_t>();
        fd_launch_pack_cands(A.cands, n, ka, va, st);
        int bits = 17;
        while (bits < 32 && (1ull << (bits - 16)) < std::max<uint64_t>(I.n_cand, 2)) ++bits;
        const int cur = sort_pairs(c, ka, va, kb, vb, n, bits);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hk, cur ? kb : ka, n * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(hv, cur ? vb : va, n * 4, hipMemcpyDeviceToHost, st));
    }
    if (T.found) HIPCHK(c, hipMemcpyAsync(hf.get(), A.found, T.found * sizeof(fd_pair_rec), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    F.tr.line("match_pairs", "packed copy done");
    fd_sort_found(hf.get(), T.found, I.n_cand);
    F.tr.line("match_pairs", "found sorted");
    *O.found = hf.release(); *O.n_found = T.found; *O.cands = nullptr; *O.n_cands = n; *I.rq.pk_key = hk; *I.rq.pk_val = hv;
    return FDGPU_OK;
}

// many found triples and no candidate pairs to keep (first scan of a large query: ~10^5 triples, most of them in the slot of the query's own
// structure): (slot, i, j) order is made on the device — two stable radix sorts over the record index, the records gathered into ws[WS_IDS_A] —
// instead of one host thread's stable_sort of that slot
static bool mp_sorts_found_on_device(const mp_in &I, const mp_form &F, const mp_totals &T) {
    uint64_t max_len = 0;
    for (uint64_t k = 0; k < I.n_cand; ++k) max_len = std::max<uint64_t>(max_len, I.db->h_res_off[I.cand[k] + 1] - I.db->h_res_off[I.cand[k]]);
    return T.found >= F.found_sort_min && T.cands == 0 && I.n_cand < 65536 && max_len < 65536 && !F.found_sort_host;
}
static int mp_sort_found_on_device(const mp_in &I, const mp_args &A, uint64_t n) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    const int rcs = mp_sort_scratch(c, n);
    if (rcs) return rcs;
    HIPCHK(c, c->ws[WS_IDS_A].ensure(n * sizeof(fd_pair_rec)));
    uint32_t *ka = c->ws[WS_MISC2].as<uint32_t>(), *va = c->ws[WS_MISC3].as<uint32_t>(), *kb = c->ws[WS_MISC4].as<uint32_t>(), *vb = c->ws[WS_MISC5].as<uint32_t>();
    fd_launch_found_key_ij(A.found, n, ka, va, st);
    int cur = sort_pairs(c, ka, va, kb, vb, n, 32);
    uint32_t *k1 = cur ? kb : ka, *v1 = cur ? vb : va, *k2 = cur ? ka : kb, *v2 = cur ? va : vb;
    fd_launch_found_key_slot(A.found, v1, n, k1, st);
    int bits = 1;
    while (bits < 16 && (1ull << bits) < std::max<uint64_t>(I.n_cand, 2)) ++bits;
    cur = sort_pairs(c, k1, v1, k2, v2, n, bits);
    fd_launch_found_gather(A.found, cur ? v2 : v1, n, c->ws[WS_IDS_A].as<fd_pair_rec>(), st);
    HIPCHK(c, hipGetLastError());
    return FDGPU_OK;
}

// found triples and candidate pairs to the host as records, in the reference's scan order (row-major over the prefilter sets, retrieve.rs:146-153):
// the kernel appends with atomics, one contiguous run per (i, j) in observed-list order
static int mp_out_records(const mp_in &I, const mp_form &F, const mp_args &A, const mp_totals &T, const mp_out &O) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    const bool sorted_on_device = mp_sorts_found_on_device(I, F, T);
    if (sorted_on_device) { const int rcs = mp_sort_found_on_device(I, A, T.found); if (rcs) return rcs; }
    mp_host<fd_pair_rec> hf = mp_host_alloc<fd_pair_rec>(T.found);
    mp_host<fd_cand_rec> hc = mp_host_alloc<fd_cand_rec>(T.cands);
    if (!hf || !hc) return FDGPU_ENOMEM;
    if (T.found) HIPCHK(c, hipMemcpyAsync(hf.get(), sorted_on_device ? c->ws[WS_IDS_A].p : (const void *)A.found, T.found * sizeof(fd_pair_rec), hipMemcpyDeviceToHost, st));
    if (T.cands) HIPCHK(c, hipMemcpyAsync(hc.get(), A.cands, T.cands * sizeof(fd_cand_rec), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    F.tr.line("match_pairs", "copy done");
    if (!sorted_on_device) fd_sort_found(hf.get(), T.found, I.n_cand);
    F.tr.line("match_pairs", "found sorted", "%s", sorted_on_device ? " (on the device)" : "");
    // MP_CANDS_UNORDERED: the caller buckets the candidate pairs itself and does not depend on their order (the rescue only counts them)
    if (!(I.rq.mode & MP_CANDS_UNORDERED)) std::stable_sort(hc.get(), hc.get() + T.cands, [](const fd_cand_rec &a, const fd_cand_rec &b) {
        if (a.cand != b.cand) return a.cand < b.cand;
        if (a.i != b.i) return a.i < b.i;
        return a.j < b.j;
    });
    *O.found = hf.release(); *O.n_found = T.found; *O.cands = hc.release(); *O.n_cands = T.cands;
    return FDGPU_OK;
}

// Pair scan for MANY queries in one launch: query t scans the candidates cand[cand_off[t] .. cand_off[t+1]); the records carry the
// GLOBAL slot (position in cand) and come back sorted by (slot, i, j).
int fd_match_pairs_multi(fdgpu_ctx *c, const fdgpu_batch *db, const uint8_t *resname_std, uint64_t n_queries, const fd_match_query *qs,
                         const uint32_t *cand, const uint64_t *cand_off, const fd_hash_params *p, fd_pair_rec **found, uint64_t *n_found,
                         fd_cand_rec **cands, uint64_t *n_cands, const fd_mp_request &rq) {
    mp_in I = {c, db, resname_std, n_queries, qs, cand, cand_off, p, rq, 0};
    const mp_out O = {found, n_found, cands, n_cands};
    mp_form F;
    int rc;
    if ((rc = mp_choose_form(I, O, F))) return rc;
    fd_mp_tables tb_local;
    fd_mp_tables &TB = rq.tables ? *rq.tables : tb_local;
    if (!TB.valid && (rc = mp_host_tables(I, F, TB))) return rc;
    F.tr.line("match_pairs", "tables", " (%zu work items)", TB.nw);
    mp_args A;
    memset(&A, 0, sizeof A);
    A.mode = rq.mode;
    mp_vote_layout VL;
    mp_totals T;
    if ((rc = mp_upload_tables(I, TB, A))) return rc;
    if ((rq.mode & MP_VOTES) && (rc = mp_upload_votes(I, VL, A))) return rc;
    if ((rc = mp_fill_args(I, TB, A))) return rc;
    if ((rc = mp_scan(I, TB.nw, A, T))) return rc;
    F.tr.line("match_pairs", "scan done", " (found %llu, cands %llu)", (unsigned long long)T.found, (unsigned long long)T.cands);
    if (rq.mode & MP_VOTES) return mp_vote_rows(I, F, VL, A);
    if (rq.mode & MP_ON_DEVICE) return mp_out_on_device(T, O);
    if (rq.pk_key) *rq.pk_key = nullptr;
    if (rq.pk_val) *rq.pk_val = nullptr;
    return mp_packs(I, F, T) ? mp_out_packed(I, F, A, T, O) : mp_out_records(I, F, A, T, O);
}
extern "C" int fdgpu_match_pairs(fdgpu_ctx *c, const fdgpu_batch *db, const uint8_t *resname_std, const uint32_t *cand, uint64_t n_cand,
                                 const fd_match_query *q, const fd_hash_params *p, fd_pair_rec **found, uint64_t *n_found,
                                 fd_cand_rec **cands, uint64_t *n_cands) { FD_LOCK(c);
    if (!q) return FDGPU_EINVAL;
    const uint64_t off[2] = {0, n_cand};
    return fd_match_pairs_multi(c, db, resname_std, 1, q, cand, off, p, found, n_found, cands, n_cands);
}

// the point lists of n superposition problems on the device: a -> ws[WS_MISC0], b -> ws[WS_MISC1] (xyz f32), off -> ws[WS_MISC2] (n + 1 entries)
static int fd_upload_problems(fdgpu_ctx *c, const float *a, const float *b, const uint64_t *off, uint64_t n) {
    hipStream_t st = c->stream;
    const uint64_t npts = off[n];
    HIPCHK(c, c->ws[WS_MISC0].ensure(std::max<uint64_t>(npts, 1) * 12));
    HIPCHK(c, c->ws[WS_MISC1].ensure(std::max<uint64_t>(npts, 1) * 12));
    HIPCHK(c, c->ws[WS_MISC2].ensure((n + 1) * 8));
    if (npts) {
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC0].p, a, npts * 12, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC1].p, b, npts * 12, hipMemcpyHostToDevice, st));
    }
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC2].p, off, (n + 1) * 8, hipMemcpyHostToDevice, st));
    return FDGPU_OK;
}

// Similarity metrics of n superpositions on the device (k_metrics): problem k compares ref[off[k] .. off[k+1]) (fixed points) with
// rot[k] * mov[...] + tran[k]; metrics[5k ..] = {tm_score, gdt_ts, gdt_ha, chamfer, hausdorff} (src/structure/metrics.rs:62-251).
extern "C" int fdgpu_metrics_batch(fdgpu_ctx *c, const float *ref, const float *mov, const uint64_t *off, uint64_t n, const float *rot, const float *tran,
                                   float *metrics) { FD_LOCK(c);
    if (!c || (n && (!ref || !mov || !off || !rot || !tran || !metrics))) return FDGPU_EINVAL;
    if (!n) return FDGPU_OK;
    hipStream_t st = c->stream;
    const uint64_t npts = off[n];
    std::vector<float> d0(n);
    for (uint64_t k = 0; k < n; ++k) {   // d0_scale (metrics.rs:117-123) with the host's powf, like the reference
        const uint64_t len = off[k + 1] - off[k];
        d0[k] = len > 21 ? 1.24f * powf((float)len - 15.0f, 1.0f / 3.0f) - 1.8f : 0.5f;
    }
    const int rcu = fd_upload_problems(c, ref, mov, off, n);
    if (rcu) return rcu;
    HIPCHK(c, c->ws[WS_MISC3].ensure(n * 4));
    HIPCHK(c, c->ws[WS_MISC4].ensure(n * 36));
    HIPCHK(c, c->ws[WS_MISC5].ensure(n * 12));
    HIPCHK(c, c->ws[WS_TILE_PO].ensure(n * 20));
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC3].p, d0.data(), n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC4].p, rot, n * 36, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC5].p, tran, n * 12, hipMemcpyHostToDevice, st));
    fd_launch_metrics(c->ws[WS_MISC0].as<float>(), c->ws[WS_MISC1].as<float>(), c->ws[WS_MISC2].as<uint64_t>(), n, c->ws[WS_MISC4].as<float>(),
                      c->ws[WS_MISC5].as<float>(), c->ws[WS_MISC3].as<float>(), c->ws[WS_TILE_PO].as<float>(), st, npts);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(metrics, c->ws[WS_TILE_PO].p, n * 20, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDGPU_OK;
}

extern "C" int fdgpu_kabsch_batch(fdgpu_ctx *c, const float *x, const float *y, const uint64_t *off, uint64_t n, float *rmsd, float *rot,
                                  float *tran) { FD_LOCK(c);
    if (!c || (n && (!x || !y || !off || !rmsd || !rot || !tran))) return FDGPU_EINVAL;
    if (!n) return FDGPU_OK;
    hipStream_t st = c->stream;
    uint64_t npts = off[n];
    const fd_call_trace tr = fd_call_trace::from_env();
    if (tr.on) { (void)hipStreamSynchronize(st); fprintf(stderr, "[kabsch] entry sync %.3f ms, %llu problems, %llu points\n", tr.ms(), (unsigned long long)n, (unsigned long long)npts); }
    const int rcu = fd_upload_problems(c, x, y, off, n);
    if (rcu) return rcu;
    HIPCHK(c, c->ws[WS_MISC3].ensure(n * 4));
    HIPCHK(c, c->ws[WS_MISC4].ensure(n * 36));
    HIPCHK(c, c->ws[WS_MISC5].ensure(n * 12));
    fd_launch_kabsch(c->ws[WS_MISC0].as<float>(), c->ws[WS_MISC1].as<float>(), c->ws[WS_MISC2].as<uint64_t>(), n, c->ws[WS_MISC3].as<float>(),
                     c->ws[WS_MISC4].as<float>(), c->ws[WS_MISC5].as<float>(), st, npts);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(rmsd, c->ws[WS_MISC3].p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(rot, c->ws[WS_MISC4].p, n * 36, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(tran, c->ws[WS_MISC5].p, n * 12, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (tr.on) fprintf(stderr, "[kabsch] total %.3f ms\n", tr.ms());
    return FDGPU_OK;
}

// --partial-fit: LmsQcpSuperimposer with its default parameters (src/structure/lms_qcp.rs), one wavefront per problem
extern "C" int fdgpu_lms_qcp_batch(fdgpu_ctx *c, const float *x, const float *y, const uint64_t *off, uint64_t n, float *rmsd, float *rot,
                                   float *tran, uint32_t *core_len, uint32_t *core) { FD_LOCK(c);
    if (!c || (n && (!x || !y || !off || !rmsd || !rot || !tran))) return FDGPU_EINVAL;
    if (!n) return FDGPU_OK;
    for (uint64_t k = 0; k < n; ++k)
        if (off[k + 1] < off[k] + 3 || off[k + 1] - off[k] > 0xffffffffull) {   // the reference asserts >= 3 pairs (lms_qcp.rs:84)
            c->err = "fdgpu_lms_qcp_batch: every problem needs at least 3 point pairs";
            return FDGPU_EINVAL;
        }
    hipStream_t st = c->stream;
    const uint64_t npts = off[n];
    const int rcu = fd_upload_problems(c, x, y, off, n);
    if (rcu) return rcu;
    HIPCHK(c, c->ws[WS_MISC3].ensure(n * 8));       // rmsd f32[n] | core_len u32[n]
    HIPCHK(c, c->ws[WS_MISC4].ensure(n * 48));      // rot f32[9n] | tran f32[3n]
    HIPCHK(c, c->ws[WS_MISC5].ensure(npts * 5));    // order u32[npts] | flags u8[npts]
    float *d_rmsd = c->ws[WS_MISC3].as<float>();
    uint32_t *d_core = (uint32_t *)(d_rmsd + n);
    float *d_rot = c->ws[WS_MISC4].as<float>(), *d_tran = d_rot + 9 * n;
    uint32_t *d_order = c->ws[WS_MISC5].as<uint32_t>();
    uint8_t *d_flags = (uint8_t *)(d_order + npts);
    fd_launch_lms_qcp(c->ws[WS_MISC0].as<float>(), c->ws[WS_MISC1].as<float>(), c->ws[WS_MISC2].as<uint64_t>(), n, d_rmsd, d_rot, d_tran, d_core,
                      d_flags, d_order, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(rmsd, d_rmsd, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(rot, d_rot, n * 36, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(tran, d_tran, n * 12, hipMemcpyDeviceToHost, st));
    if (core_len) HIPCHK(c, hipMemcpyAsync(core_len, d_core, n * 4, hipMemcpyDeviceToHost, st));
    if (core) HIPCHK(c, hipMemcpyAsync(core, d_order, npts * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDGPU_OK;
}
