// fd_api_count.hip — C ABI of libfdgpu.so, seam S3 (include/fdgpu.h): posting lookup, count_query in its forms (single, batch, query maps, the
// tiled motif path of k_qtile.hip / k_qscore32.hip, whole-structure slices) and the candidate selection — the orchestration of k_query.hip and the
// k_qt* kernels.  Reference: src/index/indextable.rs:53-86,421-463, src/controller/count_query.rs:82-220, src/cli/workflows/query_pdb.rs:404-411.
#include <math.h>
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

// ---- S3 ---------------------------------------------------------------------------------------------------------------
// posting lengths of nq query hashes (host array) left ON THE DEVICE in the context's WS_MISC1 (u64 [nq]); the sharded query all-reduces
// them there (fd_comm.hip).  No synchronisation.
int fd_posting_lengths_dev(fdgpu_ctx *c, const fdgpu_index *ix, const uint32_t *q_hash, uint64_t nq, uint64_t **dev_lengths) {
    hipStream_t st = c->stream;
    HIPCHK(c, c->ws[WS_MISC0].ensure(std::max<uint64_t>(nq, 1) * 4));
    HIPCHK(c, c->ws[WS_MISC1].ensure(std::max<uint64_t>(nq, 1) * 8));
    *dev_lengths = c->ws[WS_MISC1].as<uint64_t>();
    if (!nq) return FDGPU_OK;
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC0].p, q_hash, nq * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, c->ws[WS_CQ_KIDX].ensure(nq * 8));
    HIPCHK(c, c->ws[WS_CQ_NSEG].ensure(nq * 4));
    if (!ix->n_hashes) {      // an empty index: every hash is absent (length 0, no segments, list position -1)
        HIPCHK(c, hipMemsetAsync(c->ws[WS_MISC1].p, 0, nq * 8, st));
        HIPCHK(c, hipMemsetAsync(c->ws[WS_CQ_NSEG].p, 0, nq * 4, st));
        HIPCHK(c, hipMemsetAsync(c->ws[WS_CQ_KIDX].p, 0xff, nq * 8, st));
        return FDGPU_OK;
    }
    // the index remembers the length of every list (4 bytes per hash, one pass over the value bytes on the first request)
    {
        std::lock_guard<std::mutex> lk(ix->lens_mu);
        if (!ix->lens) {
            uint32_t *l = nullptr;
            HIPCHK(c, hipMalloc((void **)&l, ix->n_hashes * 4));
            fd_launch_index_lens(ix->offsets, ix->value, ix->n_hashes, l, st);
            hipError_t le = hipGetLastError();
            if (le == hipSuccess) le = hipStreamSynchronize(st);      // other contexts read it from their own streams
            if (le != hipSuccess) { (void)hipFree(l); c->err = std::string("posting lengths of the index: ") + hipGetErrorString(le); return FDGPU_EHIP; }
            ix->lens = l;
        }
    }
    fd_launch_posting_lookup(ix->hashes, ix->offsets, ix->lens, ix->n_hashes, c->ws[WS_MISC0].as<uint32_t>(), nq, c->ws[WS_MISC1].as<uint64_t>(),
                             c->ws[WS_CQ_NSEG].as<uint32_t>(), c->ws[WS_CQ_KIDX].as<long long>(), st);
    HIPCHK(c, hipGetLastError());
    return FDGPU_OK;
}
// lengths and the number of CQ_SEG-byte scoring segments of every hash (what k_cq_plan will find again), one synchronisation
// land_out != null (with kidx): when the page-locked block can be had the arrays STAY there — *land_out = [lengths u64 x nq | kidx i64 x nq | segs u32 x nq],
// valid until the context's block 3 is used again; lengths / segs / kidx are then untouched (reading the block twice — once to copy it out, once to use the
// copy — was 0.3 ms of a whole-structure query's 178 k lookups)
int fd_posting_lengths_segs(fdgpu_ctx *c, const fdgpu_index *ix, const uint32_t *q_hash, uint64_t nq, uint64_t *lengths, uint32_t *segs, long long *kidx,
                            const uint8_t **land_out) {
    if (land_out) *land_out = nullptr;
    if (!nq) return FDGPU_OK;
    uint64_t *d = nullptr;
    int rc = fd_posting_lengths_dev(c, ix, q_hash, nq, &d);
    if (rc) return rc;
    // the three arrays land in one page-locked block (a pageable destination makes every copy a staged, blocking one)
    uint8_t *land = (uint8_t *)c->host_pinned(FD_HP_UP, nq * 20);
    if (!land) {
        HIPCHK(c, hipMemcpyAsync(lengths, d, nq * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(segs, c->ws[WS_CQ_NSEG].p, nq * 4, hipMemcpyDeviceToHost, c->stream));
        if (kidx) HIPCHK(c, hipMemcpyAsync(kidx, c->ws[WS_CQ_KIDX].p, nq * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return FDGPU_OK;
    }
    HIPCHK(c, hipMemcpyAsync(land, d, nq * 8, hipMemcpyDeviceToHost, c->stream));
    if (kidx) HIPCHK(c, hipMemcpyAsync(land + nq * 8, c->ws[WS_CQ_KIDX].p, nq * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(land + nq * 16, c->ws[WS_CQ_NSEG].p, nq * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (land_out && kidx) { *land_out = land; return FDGPU_OK; }
    memcpy(lengths, land, nq * 8);
    if (kidx) memcpy(kidx, land + nq * 8, nq * 8);
    memcpy(segs, land + nq * 16, nq * 4);
    return FDGPU_OK;
}
extern "C" int fdgpu_posting_lengths(fdgpu_ctx *c, const fdgpu_index *ix, const uint32_t *q_hash, uint64_t nq, uint64_t *lengths) { FD_LOCK(c);
    if (!c || !ix || (nq && (!q_hash || !lengths))) return FDGPU_EINVAL;
    if (!nq) return FDGPU_OK;
    uint64_t *d = nullptr;
    int rc = fd_posting_lengths_dev(c, ix, q_hash, nq, &d);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(lengths, d, nq * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FDGPU_OK;
}

void fd_launch_posting_bytes(const uint32_t *hashes, const uint64_t *offsets, uint64_t H, const uint32_t *q_hash, uint64_t nq, uint64_t *bytes, hipStream_t st);
extern "C" int fdgpu_posting_bytes(fdgpu_ctx *c, const fdgpu_index *ix, const uint32_t *q_hash, uint64_t nq, uint64_t *bytes) { FD_LOCK(c);
    if (!c || !ix || (nq && (!q_hash || !bytes))) return FDGPU_EINVAL;
    if (!nq) return FDGPU_OK;
    hipStream_t st = c->stream;
    HIPCHK(c, c->ws[WS_MISC0].ensure(nq * 4));
    HIPCHK(c, c->ws[WS_MISC1].ensure(nq * 8));
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC0].p, q_hash, nq * 4, hipMemcpyHostToDevice, st));
    fd_launch_posting_bytes(ix->hashes, ix->offsets, ix->n_hashes, c->ws[WS_MISC0].as<uint32_t>(), nq, c->ws[WS_MISC1].as<uint64_t>(), st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(bytes, c->ws[WS_MISC1].p, nq * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDGPU_OK;
}

// get_entries for many hashes: ids of hash k = (*ids)[(*ids_off)[k] .. (*ids_off)[k+1])
extern "C" int fdgpu_get_entries(fdgpu_ctx *c, const fdgpu_index *ix, const uint32_t *q_hash, uint64_t nq, uint32_t **ids, uint64_t **ids_off) { FD_LOCK(c);
    if (!c || !ix || !ids || !ids_off || (nq && !q_hash)) return FDGPU_EINVAL;
    *ids = nullptr; *ids_off = nullptr;
    uint64_t *off = (uint64_t *)calloc(nq + 1, 8);
    if (!off) return FDGPU_ENOMEM;
    std::vector<uint64_t> lens(std::max<uint64_t>(nq, 1));
    int rc = fdgpu_posting_lengths(c, ix, q_hash, nq, lens.data());
    if (rc) { free(off); return rc; }
    for (uint64_t k = 0; k < nq; ++k) off[k + 1] = off[k] + lens[k];
    const uint64_t tot = off[nq];
    uint32_t *out = (uint32_t *)malloc(std::max<uint64_t>(tot, 1) * 4);
    if (!out) { free(off); return FDGPU_ENOMEM; }
    if (tot) {
        hipStream_t st = c->stream;
        hipError_t e = c->ws[WS_MISC0].ensure(nq * 4);
        if (e == hipSuccess) e = c->ws[WS_MISC1].ensure((nq + 1) * 8);
        if (e == hipSuccess) e = c->ws[WS_MISC2].ensure(tot * 4);
        if (e == hipSuccess) e = hipMemcpyAsync(c->ws[WS_MISC0].p, q_hash, nq * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(c->ws[WS_MISC1].p, off, (nq + 1) * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            fd_launch_get_entries(ix->hashes, ix->offsets, ix->value, ix->n_hashes, c->ws[WS_MISC0].as<uint32_t>(), nq, c->ws[WS_MISC1].as<uint64_t>(),
                                  c->ws[WS_MISC2].as<uint32_t>(), st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out, c->ws[WS_MISC2].p, tot * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { free(off); free(out); c->err = std::string("get_entries: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    }
    *ids = out; *ids_off = off;
    return FDGPU_OK;
}

// idf of a query hash in the accumulators' fixed point (2^-22; count_query.rs:181-200 sums f32 in hash-map order, here the sum is exact
// and order-independent to 2.4e-7 per addend)
static inline uint64_t fd_idf_fix(float idf) {
    const double v = (double)idf;
    return (v > 0.0 && v < 1.0e6) ? (uint64_t)(v * 4194304.0 + 0.5) : 0ull;
}
// The rows of one query in (node, partner) order with their metadata word: idf (2^-22 fixed point) << 2 | last row of its node << 1 |
// last row of its edge.  -> false when an idf does not fit the packed accumulator (>= 32).
static bool fd_cq_rows(const uint32_t *q_hash, const uint32_t *q_node, const uint32_t *q_edge_j, const float *q_idf, uint64_t a, uint64_t b,
                       std::vector<uint32_t> &rows_hash, std::vector<unsigned long long> &rows_meta, const long long *q_kidx = nullptr,
                       std::vector<long long> *rows_kidx = nullptr) {
    std::vector<uint64_t> ord(b - a);
    for (uint64_t k = a; k < b; ++k) ord[k - a] = k;
    bool small_ids = true, in_order = true;
    for (uint64_t k = a; k < b && small_ids; ++k) small_ids = q_node[k] < 65536u && q_edge_j[k] < 65536u;
    // a query map lists its entries pair by pair in row-major (i, j) order (query.rs:231-329): a whole-structure query's 10^5 rows arrive sorted
    for (uint64_t k = a + 1; k < b && in_order; ++k) in_order = q_node[k - 1] < q_node[k] || (q_node[k - 1] == q_node[k] && q_edge_j[k - 1] <= q_edge_j[k]);
    if (in_order) {
    } else if (b - a > 2048 && small_ids) {
        // a whole-structure query has ~10^5 rows: (node, partner) order by a stable LSD radix sort of node << 16 | partner (a comparison
        // sort of the index array took several milliseconds of the prefilter)
        std::vector<uint64_t> tmp(ord.size());
        for (int pass = 0; pass < 4; ++pass) {
            const int sh = 8 * pass;
            size_t cnt[257] = {0};
            auto key = [&](uint64_t k) { return ((q_node[k] << 16) | q_edge_j[k]) >> sh & 255u; };
            for (uint64_t k : ord) ++cnt[key(k) + 1];
            for (int d = 0; d < 256; ++d) cnt[d + 1] += cnt[d];
            for (uint64_t k : ord) tmp[cnt[key(k)]++] = k;
            ord.swap(tmp);
        }
    } else
    std::stable_sort(ord.begin(), ord.end(), [&](uint64_t x, uint64_t y) {
        return q_node[x] != q_node[y] ? q_node[x] < q_node[y] : q_edge_j[x] < q_edge_j[y];
    });
    bool fits = true;
    const size_t n = ord.size(), base = rows_hash.size();
    rows_hash.resize(base + n); rows_meta.resize(base + n);
    const bool with_k = q_kidx && rows_kidx;
    if (with_k) rows_kidx->resize(base + n);
    uint32_t *const oh = rows_hash.data() + base;
    unsigned long long *const om = rows_meta.data() + base;
    long long *const ok = with_k ? rows_kidx->data() + base : nullptr;
    const uint64_t *const od = ord.data();
    for (size_t z = 0; z < n; ++z) {
        const uint64_t k = od[z];
        const uint64_t fix = fd_idf_fix(q_idf[k]);
        fits = fits && fix < (1ull << 27);
        const bool last = z + 1 == n;
        const bool node_end = last || q_node[od[z + 1]] != q_node[k];
        const bool edge_end = node_end || q_edge_j[od[z + 1]] != q_edge_j[k];
        oh[z] = q_hash[k];
        if (ok) ok[z] = q_kidx[k];
        om[z] = ((unsigned long long)fix << 2) | (node_end ? 2ull : 0ull) | (edge_end ? 1ull : 0ull);
    }
    return fits;
}

// The index's checkpoint table for tiled scoring (k_qtile.hip), made on first use for the id range the index has then: sizes per list ->
// exclusive scan -> one sequential decode of every list long enough to hold entries.  -> FDGPU_OK with the table published, FDGPU_ENOMEM
// when it does not fit (remembered: the caller keeps the occupancy-row path for this index).
static int fd_index_checkpoints(fdgpu_ctx *c, const fdgpu_index *ix) {
    std::lock_guard<std::mutex> lk(ix->lens_mu);
    if (ix->ck_meta && ix->ck_first == ix->first_id && ix->ck_S == ix->n_structures) return FDGPU_OK;
    // a failure is remembered for the id range it happened with (a changed range is a new table of another size) and retried every 64th request:
    // one transient hipMalloc failure must not switch the tiled path off for the life of the index
    if (ix->ck_failed && ix->ck_first == ix->first_id && ix->ck_S == ix->n_structures && (++ix->ck_fail_skips & 63)) return FDGPU_ENOMEM;
    hipStream_t st = c->stream;
    const uint64_t H = ix->n_hashes, S = ix->n_structures;
    if (!H || !S) return FDGPU_ENOMEM;
    if (ix->ck_meta) {
        // the table of the previous id range: other contexts that share the index (query lanes, one context per host thread) may still have
        // k_qt_plan / k_qt_score in flight on THEIR streams reading it — drain the whole device, not only this context's stream, before the free
        (void)hipDeviceSynchronize();
        (void)hipFree(ix->ck_meta); (void)hipFree(ix->ck_ent); ix->ck_meta = nullptr; ix->ck_ent = nullptr;
    }
    ix->ck_failed = false;
    const uint32_t NC = (uint32_t)((S + (1u << QT_CELL_LOG2) - 1) >> QT_CELL_LOG2);
    hipError_t e = c->ws[WS_QT_COUNT].ensure(H * 4);
    if (e == hipSuccess) e = c->ws[WS_QT_RANGES].ensure((H + 2) * 8);
    if (e == hipSuccess) e = c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(H) * 8 + 64);
    if (e == hipSuccess) e = c->ws[WS_TOTAL].ensure(64);
    unsigned long long *meta = nullptr;
    void *ent = nullptr;
    uint64_t n_ent = 0;
    if (e == hipSuccess) {
        fd_launch_ck_count(ix->offsets, H, NC, c->ws[WS_QT_COUNT].as<uint32_t>(), st);
        fd_exclusive_scan<uint32_t>(c->ws[WS_QT_COUNT].as<uint32_t>(), H, c->ws[WS_QT_RANGES].as<uint64_t>(), c->ws[WS_SCANTMP].as<uint64_t>(),
                                    c->ws[WS_TOTAL].as<uint64_t>(), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&n_ent, c->ws[WS_TOTAL].p, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMalloc((void **)&meta, H * 8);
    if (e == hipSuccess) e = hipMalloc(&ent, std::max<uint64_t>(n_ent, 1) * 8);
    if (e == hipSuccess) {
        fd_launch_ck_fill(ix->offsets, ix->value, H, NC, (uint32_t)S, (uint32_t)ix->first_id, c->ws[WS_QT_RANGES].as<uint64_t>(), meta, ent, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // other contexts read the table from their own streams
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (meta) (void)hipFree(meta);
        if (ent) (void)hipFree(ent);
        ix->ck_failed = true; ix->ck_first = ix->first_id; ix->ck_S = S;
        return FDGPU_ENOMEM;
    }
    ix->ck_meta = meta; ix->ck_ent = ent; ix->ck_n = n_ent; ix->ck_first = ix->first_id; ix->ck_S = S;
    return FDGPU_OK;
}

// batched count_query: queries [q_off[t], q_off[t+1]) of the concatenated hash arrays; results of query t are
// (*out)[(*out_off)[t] .. (*out_off)[t+1])
// idf descending, ties by ascending structure id (the candidate ranking of query_pdb.rs:404-411), cut to top_n; -> records kept
static uint64_t fd_rank_trim(fd_count_rec *r, uint64_t n, uint32_t top_n) {
    auto key = [](const fd_count_rec &x) {
        float v = x.idf + 0.0f;
        uint32_t b; memcpy(&b, &v, 4);
        const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
        return ((uint64_t)(~o) << 32) | x.nid;
    };
    std::sort(r, r + n, [&](const fd_count_rec &a, const fd_count_rec &b) { return key(a) < key(b); });
    return std::min<uint64_t>(n, top_n);
}

// ---- the stages of a scoring call: order rows -> choose form -> reserve scratch -> upload -> score -> (select on device | compact and bring home) ----
static const uint32_t QT_TL2 = 14;                            // structures per tile: 2^14 (two workgroups per CU)
static const uint32_t QT_WPR = (1u << (QT_TL2 - 8)) + 2u;     // windows a row can need in a tile: < 2 bytes per posting of a tile, windows at least half full, + its pieces' tails

// a call's host arrays belong to these until the success exits release them to the caller
template <void (*F)(void *)> struct cq_del { void operator()(void *p) const { F(p); } };
typedef std::unique_ptr<uint64_t, cq_del<free>> cq_off_ptr;
typedef std::unique_ptr<fd_count_rec, cq_del<free>> cq_rec_ptr;
typedef std::unique_ptr<fd_count_rec, cq_del<fdgpu_free>> cq_pooled_ptr;      // fd_out_alloc's blocks

// host-side stage stamps on stderr (FDGPU_TRACE, measurement aid)
struct cq_stamps {
    const bool on = getenv("FDGPU_TRACE") != nullptr;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// occupancy rows: the query hashes of the whole batch, per query in (node, partner) order, and what the form depends on
struct cq_rows {
    std::vector<uint32_t> hash;
    std::vector<unsigned long long> meta;
    std::vector<long long> kidx;       // the rows' list positions when the caller knows them (query maps made against this index)
    bool packed = true, sums_fit32 = true;
    uint64_t max_rows = 0;
};
static void cq_order_rows(uint64_t n_queries, const uint64_t *q_off, const uint32_t *q_hash, const uint32_t *q_node, const uint32_t *q_edge_j, const float *q_idf,
                          const long long *known_kidx, cq_rows &R) {
    const uint64_t nq = q_off[n_queries];
    R.hash.reserve(nq); R.meta.reserve(nq);
    if (known_kidx) R.kidx.reserve(nq);
    for (uint64_t t = 0; t < n_queries; ++t) {
        R.max_rows = std::max<uint64_t>(R.max_rows, q_off[t + 1] - q_off[t]);
        R.packed = R.packed && (q_off[t + 1] - q_off[t]) < (1ull << 18);
        R.packed = fd_cq_rows(q_hash, q_node, q_edge_j, q_idf, q_off[t], q_off[t + 1], R.hash, R.meta, known_kidx, &R.kidx) && R.packed;
        // 32-bit accumulators serve the batch when no row adds nothing (touched <=> sum != 0) and no query's idf units can reach 2^32
        unsigned long long units = 0;
        for (uint64_t r = q_off[t]; r < q_off[t + 1]; ++r) { const unsigned long long fix = R.meta[r] >> 2; units += fix; R.sums_fit32 = R.sums_fit32 && fix != 0ull; }
        R.sums_fit32 = R.sums_fit32 && units < (1ull << 32);
    }
}

// The decisions of the dispatch.  tests/test_gpu_scoring_edges.py::expected_path restates the conditions of cq_choose_form.
struct cq_form {
    bool packed, sums_fit32; uint64_t max_rows;      // from the rows (cq_order_rows)
    bool dense_topn;            // the candidate selection runs on the dense results (no flag scan, no compaction)
    bool sliced;                // one query with thousands of rows (whole-structure mode): its rows are walked in slices
    bool keys_only;             // motif queries with a selection: no dense results at all, records only for the survivors
    bool tiled, tiled_big;      // scores per tile of structures in LDS (k_qtile.hip): motif batches / one large query (k_qt_score<BIG>)
    bool qt32;                  // k_qscore32.hip: 32-bit sums, planned slot stream
    uint64_t stream_cap;        // records of the tiled form's decoded stream (k_qt_rows), 0: pass B decodes the lists again
    uint32_t NT, NC, words; uint64_t QS;      // tiles, checkpoint cells and occupancy words of the index's S structures; n_queries x S
    uint32_t big_slices, big_wpr, cap;      // the large query's row slices and words per row bitmap; the selection's slots per query (top_n + 1024)
    bool rows_form() const { return !tiled && !tiled_big; }
    void to_rows_form() { tiled = false; tiled_big = false; qt32 = false; stream_cap = 0; }
    uint32_t path() const {
        return (tiled ? FDGPU_PATH_TILED : 0u) | (qt32 ? FDGPU_PATH_SUMS32 : 0u) | (tiled && stream_cap ? FDGPU_PATH_STREAM : 0u) |
               (tiled_big ? FDGPU_PATH_SLICED : 0u) | (rows_form() ? FDGPU_PATH_ROWS : 0u) | (packed ? FDGPU_PATH_PACKED : 0u);
    }
};
static bool cq_env_on(const char *name) { const char *e = getenv(name); return !(e && e[0] == '0'); }      // read per call: tests compare the forms
static cq_form cq_choose_form(fdgpu_ctx *c, const fdgpu_index *ix, const cq_rows &R, uint64_t n_queries, uint64_t nq, uint32_t top_n, bool allow_dense,
                              const uint64_t *known_len) {
    const uint64_t S = ix->n_structures;
    cq_form F = {};
    F.packed = R.packed; F.sums_fit32 = R.sums_fit32; F.max_rows = R.max_rows;
    F.words = (uint32_t)((S + 31) / 32);
    F.QS = n_queries * S;
    F.cap = top_n + 1024;
    F.dense_topn = allow_dense && F.packed && top_n > 0 && top_n + 1024 <= 4096;
    // one query with thousands of rows (whole-structure mode): its rows are walked in slices that add into the dense results; motif
    // queries with a selection skip the dense results altogether: scores per tile of structures in LDS (k_qtile.hip), or, when the
    // index has no checkpoint table, ranking keys from occupancy rows (k_cq_rows_keys); records only for the survivors either way
    F.sliced = n_queries == 1 && nq >= 4096;
    F.keys_only = F.dense_topn && !F.sliced;
    const bool qtile_on = cq_env_on("FDGPU_QTILE");       // 0: occupancy rows
    // k_qscore32.hip needs the rows' posting lengths for the stream's bound; FDGPU_QT32=0 keeps the 64-bit kernel
    // (queries of more than 128 rows keep the 64-bit kernel as well: their idf units reach 2^32 on any real index, and k_qt_rows' small tables are sized for 128)
    F.qt32 = F.keys_only && qtile_on && cq_env_on("FDGPU_QT32") && F.sums_fit32 && known_len && F.max_rows <= 128;
    F.NT = (uint32_t)((S + (1u << QT_TL2) - 1) >> QT_TL2);
    F.NC = (uint32_t)((S + (1u << QT_CELL_LOG2) - 1) >> QT_CELL_LOG2);
    F.tiled = F.keys_only && qtile_on && F.max_rows <= QT_MAX_ROWS && nq * (S >> QT_CELL_LOG2) < (1ull << 31) && fd_index_checkpoints(c, ix) == FDGPU_OK;
    F.qt32 = F.qt32 && F.tiled;
    // one query of thousands of rows (a whole structure as the query) with a selection: the same tiles, the rows cut into slices (k_qt_score<BIG>)
    F.tiled_big = F.dense_topn && F.sliced && qtile_on && !F.tiled && nq < (1ull << 18) && nq * F.NT < (1ull << 31) && fd_index_checkpoints(c, ix) == FDGPU_OK;
    F.big_slices = (uint32_t)std::min<uint64_t>(32, nq); F.big_wpr = (uint32_t)((nq + 31) / 32);
    // the decoded stream of the tiled path (k_qt_rows): sized from the rows' posting lengths when the caller knows them — a list of n ids is at most
    // n x (bytes of the largest id) bytes, a slot holds 16 of them, and every (row, cell) piece ends in one partly filled slot
    // (FDGPU_QT_STREAM=0: pass B decodes the lists again — tests, measurement)
    if (F.tiled && (F.qt32 || (cq_env_on("FDGPU_QT_STREAM") && known_len && F.max_rows * (1u << (QT_TL2 - QT_CELL_LOG2)) <= (uint64_t)QT_MAXB * 512))) {
        const uint64_t top_id = ix->first_id + S, vb = top_id < (1ull << 7) ? 1 : top_id < (1ull << 14) ? 2 : top_id < (1ull << 21) ? 3 : top_id < (1ull << 28) ? 4 : 5;
        // a piece per (row, cell) where the list has an entry per cell; a list with entries 2^j cells apart is cut into pieces of < 96 bytes on
        // average that every tile they span decodes once: at most 6 slots x tiles on top of its bytes
        uint64_t slots = 0;
        for (uint64_t r = 0; r < nq; ++r) slots += (known_len[r] * vb + 15) / 16 + F.NC + 6ull * F.NT + 8;
        // (the planned stream pads its windows: a piece that would straddle a 64-slot boundary starts the next window — windows stay at least half full)
        if (F.qt32) slots = 2 * slots + 64ull * n_queries * F.NT;
        if (slots < (1ull << 31)) F.stream_cap = slots + 1024;
        else F.qt32 = false;
        // FDGPU_QT_STREAM_CAP=n (tests): a stream of n records — the tiles that do not fit raise the selection's overflow flag and the call is ranked by the compacting path
        if (const char *e = getenv("FDGPU_QT_STREAM_CAP")) { const long v = atol(e); if (v > 0 && (uint64_t)v < F.stream_cap) F.stream_cap = (uint64_t)v; }
    }
    return F;
}

// The device arrays of a scoring call.  cq_reserve fills all of them; the stages below never name a workspace slot.
struct cq_scratch {
    uint32_t *q_hash; unsigned long long *row_meta; uint64_t *q_off; float *penalty; uint8_t *in_block;      // the call's inputs
    long long *kidx; uint32_t *nseg; uint64_t *wstart, *scan_tmp, *total;                                    // plan: list positions, segments, scans
    uint32_t *match; unsigned long long *idf; uint32_t *occupancy, *node_cnt, *edge_cnt; uint8_t *flags; uint64_t *pos; uint32_t *keys; uint64_t *slices;     // rows form
    uint4 *ranges; uint32_t *compact, *tile_cnt; qt_aux *aux; uint8_t *stream, *stream_tab; uint32_t *piece_p, *win; uint4 *heads;                        // tiled forms
    unsigned long long *partial; uint32_t *surv, *rowbits;                                                   // ... one large query
    void *sel, *ranked; qt_state *sel_state; uint32_t *ghist;                                                // candidate selection
    void *records; uint64_t *rec_off, *gather_idx;                                                           // compaction
};
// The selection's scratch — sel: cap slots per query (WS_KEYS_A), sel_state (WS_MISC2), ghist (WS_CQ_TOPN), ranked: top_n records per query — for the selection
// on the dense results (ranked in WS_TILE_HO) and for the one after a compaction (in WS_KEYS_B, or none: ranked on the host).  The histogram table is zeroed
// when it grows; the kernels leave it zero.
static hipError_t cq_reserve_selection(fdgpu_ctx *c, uint64_t n_queries, uint32_t top_n, uint32_t cap, int ranked_slot, cq_scratch &W) {
    hipError_t e = c->ws[WS_KEYS_A].ensure((size_t)n_queries * cap * sizeof(fd_count_rec));
    if (e == hipSuccess && ranked_slot >= 0) e = c->ws[ranked_slot].ensure((size_t)n_queries * top_n * sizeof(fd_count_rec));
    const size_t topn_bytes = (size_t)n_queries * 2048 * 4;
    if (e == hipSuccess && c->ws[WS_CQ_TOPN].cap < topn_bytes) {
        e = c->ws[WS_CQ_TOPN].ensure(topn_bytes);
        if (e == hipSuccess) e = hipMemsetAsync(c->ws[WS_CQ_TOPN].p, 0, c->ws[WS_CQ_TOPN].cap, c->stream);
    }
    if (e == hipSuccess) e = c->ws[WS_MISC2].ensure(n_queries * 16);
    W.sel = c->ws[WS_KEYS_A].p; W.ranked = ranked_slot >= 0 ? c->ws[ranked_slot].p : nullptr;
    W.ghist = c->ws[WS_CQ_TOPN].as<uint32_t>(); W.sel_state = c->ws[WS_MISC2].as<qt_state>();
    return e;
}
// the compacted records (WS_TILE_HO, like the device selection's ranked records: never both in one call): their number is known only after the flag scan's synchronisation
static hipError_t cq_reserve_records(fdgpu_ctx *c, uint64_t n, cq_scratch &W) {
    const hipError_t e = c->ws[WS_TILE_HO].ensure(std::max<uint64_t>(n, 1) * sizeof(fd_count_rec));
    W.records = c->ws[WS_TILE_HO].p;
    return e;
}
// Every ensure() a form needs (cq_score's segment sums, cq_reserve_records and the selection after a compaction excepted: their sizes come from a
// synchronisation).  A tiled form whose scratch does not fit (ranges, first-touch lists, decoded stream) becomes the rows form.  Pointers are taken
// after the last ensure() of their slot.  Slots that serve two arrays do so because the arrays never live at the same time (the table at the end).
static int cq_reserve(fdgpu_ctx *c, cq_form &F, uint64_t n_queries, uint64_t nq, uint64_t S, uint32_t top_n, cq_scratch &W) {
    hipError_t e = hipSuccess;
    auto need = [&](int w, size_t bytes) { if (e == hipSuccess) e = c->ws[w].ensure(bytes); };
    auto form_scratch = [&]() {
        e = hipSuccess;
        need(WS_MISC0, nq * 4); need(WS_MISC3, F.tiled ? 2 * nq * 8 + (n_queries + 1) * 8 + nq * 4 + 64 : nq * 8);
        need(WS_TILE_H, (n_queries + 1) * 8); need(WS_MISC5, S * 4); need(WS_TOTAL, 64);
        need(WS_CQ_KIDX, nq * 8); need(WS_CQ_NSEG, nq * 4);
        if (F.tiled) {
            if (F.stream_cap) { need(WS_QT_STREAM, F.stream_cap * 34 + 64); need(WS_QT_STAB, (size_t)n_queries * F.NT * QT_MAXB * 8 + 64); }
            need(WS_QT_RANGES, (size_t)nq * F.NC * 16); need(WS_QT_COMPACT, ((size_t)n_queries * F.NT << QT_TL2) * 8);
            need(WS_QT_COUNT, (size_t)n_queries * F.NT * 4); need(WS_QT_AUX, n_queries * sizeof(qt_aux) + 256);
            if (F.qt32) {       // pieces in WS_QT_RANGES ([nq x NT x cells per tile] >= the ranges table), their first slots, the window tables, the heads
                const size_t ent = (size_t)nq * F.NT << (QT_TL2 - QT_CELL_LOG2);
                need(WS_QT_RANGES, ent * 16); need(WS_QT_PIECEP, ent * 4);
                need(WS_QT_WIN, ((size_t)nq * F.NT * QT_WPR + 2 * (size_t)n_queries * F.NT) * 4); need(WS_QT_HEAD, (size_t)n_queries * F.NT * 16);
            }
        } else if (F.tiled_big) {
            need(WS_QT_RANGES, (size_t)nq * F.NT * 16); need(WS_QT_COMPACT, ((size_t)F.NT << QT_TL2) * 8); need(WS_QT_COUNT, (size_t)F.NT * 4); need(WS_QT_AUX, sizeof(qt_aux) + 256);
            need(WS_QT_PARTIAL, ((size_t)F.big_slices * F.NT << QT_TL2) * 8);
            need(WS_QT_SURV, ((size_t)F.NT * 512 * 2 + F.NT + F.cap + 2 * F.big_wpr) * 4 + (F.big_slices + 2) * 8 + 64);
            need(WS_QT_ROWBITS, (size_t)F.cap * F.big_wpr * 4);
        } else {
            need(WS_CQ_WSTART, (nq + 2) * 8);
            need(WS_COUNTS, F.packed ? 64 : F.QS * 4); need(WS_SEGOFF, F.QS * 8 + 16);
            need(WS_KEYS_B, (size_t)nq * F.words * 4);
            need(WS_IDS_A, F.QS * 4); need(WS_IDS_B, F.QS * 4); need(WS_MISC4, F.QS + 8); need(WS_TILE_BO, (F.QS + 2) * 8);
            need(WS_SCANTMP, std::max(fd_scan_tmp_elems(F.QS), fd_scan_tmp_elems(nq)) * 8 + 64);
            if (F.sliced) need(WS_TILE_B, 40 * 8);      // at most 32 slices of >= nq / 32 rows and the two ends
            if (!F.dense_topn) { need(WS_TILE_PO, (n_queries + 1) * 8 + 64); need(WS_MISC1, (n_queries + 1) * 8); }
        }
    };
    form_scratch();
    if (e != hipSuccess && !F.rows_form()) { (void)hipGetLastError(); F.to_rows_form(); form_scratch(); }
    if (e != hipSuccess) { c->err = std::string("count_query_batch workspace: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    if (F.dense_topn && (e = cq_reserve_selection(c, n_queries, top_n, F.cap, WS_TILE_HO, W)) != hipSuccess) { c->err = std::string("count_query_batch: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    // slot by slot: what the array holds, and the forms that need it.  (The selection's slots: cq_reserve_selection; the records in WS_TILE_HO: cq_reserve_records.)
    fd_devbuf *const ws = c->ws;
    W.q_hash = ws[WS_MISC0].as<uint32_t>();                  // row hashes (inside in_block after a packed upload)
    W.row_meta = ws[WS_MISC3].as<unsigned long long>(); W.in_block = ws[WS_MISC3].as<uint8_t>();      // row metadata | tiled: the one-copy block [metadata | list positions | row ranges | hashes]
    W.q_off = ws[WS_TILE_H].as<uint64_t>(); W.penalty = ws[WS_MISC5].as<float>(); W.total = ws[WS_TOTAL].as<uint64_t>();      // the queries' row ranges, the caller's length penalty, a scan's total
    W.kidx = ws[WS_CQ_KIDX].as<long long>(); W.nseg = ws[WS_CQ_NSEG].as<uint32_t>();                  // the rows' list positions and CQ_SEG-byte segments
    W.wstart = ws[WS_CQ_WSTART].as<uint64_t>(); W.scan_tmp = ws[WS_SCANTMP].as<uint64_t>();           // rows: first work item of every row; block sums of the scans over rows and over the flags
    W.match = ws[WS_COUNTS].as<uint32_t>(); W.idf = ws[WS_SEGOFF].as<unsigned long long>();           // rows: match counts of the wide form; idf sums (packed: count << 46 | sum)
    W.occupancy = ws[WS_KEYS_B].as<uint32_t>();              // rows: occupancy rows, dead once the flags are made | then the ranked selection after a compaction
    W.node_cnt = ws[WS_IDS_A].as<uint32_t>(); W.edge_cnt = ws[WS_IDS_B].as<uint32_t>(); W.flags = ws[WS_MISC4].as<uint8_t>();      // rows: per (query, structure); touched
    W.pos = ws[WS_TILE_BO].as<uint64_t>(); W.keys = ws[WS_TILE_BO].as<uint32_t>();                    // rows: scan of the flags | keys_only: ranking keys (no compaction, no positions)
    W.slices = ws[WS_TILE_B].as<uint64_t>();                 // rows, sliced: row slices of the one large query
    W.ranges = ws[WS_QT_RANGES].as<uint4>();                 // tiled, tiled_big: byte ranges per (row, cell); qt32: the pieces
    W.compact = ws[WS_QT_COMPACT].as<uint32_t>(); W.tile_cnt = ws[WS_QT_COUNT].as<uint32_t>(); W.aux = ws[WS_QT_AUX].as<qt_aux>();      // tiled, tiled_big: touched structures and keys per tile
    W.stream = ws[WS_QT_STREAM].as<uint8_t>(); W.stream_tab = ws[WS_QT_STAB].as<uint8_t>();           // tiled with stream_cap: the decoded stream and its tables
    W.piece_p = ws[WS_QT_PIECEP].as<uint32_t>(); W.win = ws[WS_QT_WIN].as<uint32_t>(); W.heads = ws[WS_QT_HEAD].as<uint4>();             // tiled with qt32
    W.partial = ws[WS_QT_PARTIAL].as<unsigned long long>(); W.surv = ws[WS_QT_SURV].as<uint32_t>(); W.rowbits = ws[WS_QT_ROWBITS].as<uint32_t>();      // tiled_big
    W.rec_off = ws[WS_TILE_PO].as<uint64_t>(); W.gather_idx = ws[WS_MISC1].as<uint64_t>();            // compaction: the queries' first records, read from the flag scan at t x S
    return FDGPU_OK;
}

// The rows' inputs on the device: hashes, metadata, the queries' row ranges and — when the caller knows them — the rows' list positions.  The tiled motif
// form sends them up in ONE block packed in page-locked memory ([metadata | list positions | row ranges | hashes] in W.in_block): one copy launch, not four.
struct cq_inputs { const uint32_t *q_hash; const unsigned long long *row_meta; const uint64_t *q_off; long long *kidx; const float *penalty; bool have_k; };
static cq_inputs cq_upload(fdgpu_ctx *c, const fdgpu_index *ix, const cq_form &F, const cq_scratch &W, const cq_rows &R, uint64_t n_queries, const uint64_t *q_off,
                           const float *penalty, bool have_k) {
    hipStream_t st = c->stream;
    const uint64_t nq = q_off[n_queries];
    cq_inputs In = {W.q_hash, W.row_meta, W.q_off, W.kidx, penalty ? W.penalty : ix->penalty, have_k};
    const size_t o_k = nq * 8, o_off = 2 * nq * 8, o_h = o_off + (n_queries + 1) * 8, up_bytes = o_h + nq * 4;
    uint8_t *up = F.tiled ? (uint8_t *)c->host_pinned(FD_HP_PAIRS, up_bytes) : nullptr;
    bool k_up = false;      // the list positions went up with the block
    if (up) {
        memcpy(up, R.meta.data(), nq * 8);
        if (have_k) memcpy(up + o_k, R.kidx.data(), nq * 8);
        memcpy(up + o_off, q_off, (n_queries + 1) * 8);
        memcpy(up + o_h, R.hash.data(), nq * 4);
        uint8_t *d_blk = W.in_block;
        In.row_meta = (unsigned long long *)d_blk; In.kidx = (long long *)(d_blk + o_k); In.q_off = (uint64_t *)(d_blk + o_off); In.q_hash = (uint32_t *)(d_blk + o_h);
        (void)hipMemcpyAsync(d_blk, up, up_bytes, hipMemcpyHostToDevice, st);
        k_up = have_k;
    } else {
        (void)hipMemcpyAsync(W.q_hash, R.hash.data(), nq * 4, hipMemcpyHostToDevice, st);
        (void)hipMemcpyAsync(W.row_meta, R.meta.data(), nq * 8, hipMemcpyHostToDevice, st);
        (void)hipMemcpyAsync(W.q_off, q_off, (n_queries + 1) * 8, hipMemcpyHostToDevice, st);
    }
    if (penalty) (void)hipMemcpyAsync(W.penalty, penalty, ix->n_structures * 4, hipMemcpyHostToDevice, st);
    // (the tiled forms take the rows' list positions as an input like their hashes: uploaded before the timed stage)
    if (!F.rows_form() && have_k && !k_up) (void)hipMemcpyAsync(In.kidx, R.kidx.data(), nq * 8, hipMemcpyHostToDevice, st);
    return In;
}
static cq_args cq_row_args(const fdgpu_index *ix, const cq_form &F, const cq_scratch &W, const cq_inputs &In, uint64_t nq) {
    cq_args A;
    A.hashes = ix->hashes; A.offsets = ix->offsets; A.value = ix->value; A.H = ix->n_hashes;
    A.q_hash = In.q_hash; A.nq = nq; A.hash_bits = W.occupancy; A.row_meta = In.row_meta;
    A.match = W.match; A.idf = W.idf; A.packed = F.packed ? 1 : 0;
    A.words = F.words; A.first_id = (uint32_t)ix->first_id; A.S = (uint32_t)ix->n_structures;
    return A;
}

// what both tiled forms pass their kernels; the motif form adds the stream, pieces and windows, the large query its slices, partial sums and survivors
static qt_args cq_tile_args(const fdgpu_index *ix, const cq_form &F, const cq_scratch &W, const cq_inputs &In, uint64_t nq, uint64_t n_queries, uint32_t top_n) {
    qt_args T = {};
    T.value = ix->value; T.offsets = ix->offsets; T.ck_meta = ix->ck_meta; T.ck_ent = (const uint2 *)ix->ck_ent;
    T.kidx = In.kidx; T.row_meta = In.row_meta; T.q_rows = In.q_off; T.penalty = In.penalty;
    T.nq = (uint32_t)nq; T.n_queries = (uint32_t)n_queries; T.S = (uint32_t)ix->n_structures; T.first_id = (uint32_t)ix->first_id;
    T.NT = F.NT; T.NC = F.NC; T.tile_log2 = QT_TL2; T.plan_log2 = F.tiled_big ? QT_TL2 : QT_CELL_LOG2;
    T.ranges = W.ranges; T.c_nid = W.compact; T.c_key = T.c_nid + ((size_t)n_queries * F.NT << QT_TL2); T.ccount = W.tile_cnt; T.aux = W.aux;
    T.ghist = W.ghist; T.state = W.sel_state; T.out = W.sel; T.cap = F.cap; T.top_n = top_n; T.max_rows = (uint32_t)F.max_rows;
    return T;
}
static void cq_motif_args(fdgpu_ctx *c, const cq_form &F, const cq_scratch &W, uint64_t n_queries, qt_args &T) {
    if (F.stream_cap) {
        T.stream_ids = W.stream; T.stream_row = (uint16_t *)(W.stream + F.stream_cap * 32); T.stream_cap = (uint32_t)F.stream_cap;
        T.stream_tab = (uint2 *)W.stream_tab; T.stream_used = (uint32_t *)(W.stream_tab + (size_t)n_queries * F.NT * QT_MAXB * 8);
        if (!F.qt32) (void)hipMemsetAsync(T.stream_used, 0, 4, c->stream);       // (the 32-bit path scans the tiles' windows instead of claiming records: k_qt_bases)
    }
    if (F.qt32) { T.pieces = W.ranges; T.piece_p = W.piece_p; T.win = W.win; T.heads = W.heads; T.win_per_row = QT_WPR; }
}
// The large query's host work: row slices of roughly equal posting counts — a row's list holds ~ S / 2^idf ids (idf = log2(S / length), its fixed-point
// image is in the metadata) — and the bitmaps of the rows that end an edge / a node.
static void cq_big_slices(const std::vector<unsigned long long> &meta, const cq_form &F, std::vector<uint64_t> &sl, std::vector<uint32_t> &ends) {
    const uint64_t nq = meta.size();
    std::vector<double> w(nq);
    double tot = 0;
    for (uint64_t r = 0; r < nq; ++r) {       // 2^-idf to a few percent: the integer part as an exponent field, the fraction linearly
        const unsigned long long fix = meta[r] >> 2;
        const uint64_t eb = (uint64_t)(1023 - (int)std::min<unsigned long long>(fix >> 22, 1000ull)) << 52;
        double p2;
        memcpy(&p2, &eb, 8);
        w[r] = (1.0 - 0.5 * (double)(fix & 4194303ull) / 4194304.0) * p2 + 1e-7;
        tot += w[r];
    }
    sl.push_back(0);
    double acc = 0;
    for (uint64_t r = 0; r < nq; ++r) {
        acc += w[r];
        if (sl.size() < F.big_slices && acc >= tot * (double)sl.size() / F.big_slices && r + 1 < nq) sl.push_back(r + 1);
    }
    sl.push_back(nq);
    ends.assign((size_t)2 * F.big_wpr, 0u);
    for (uint64_t r = 0; r < nq; ++r) {
        if (meta[r] & 1ull) ends[r >> 5] |= 1u << (r & 31u);
        if (meta[r] & 2ull) ends[F.big_wpr + (r >> 5)] |= 1u << (r & 31u);
    }
}
// sl, ends: the caller's, they outlive their asynchronous copies
static void cq_big_args(fdgpu_ctx *c, const cq_form &F, const cq_scratch &W, const std::vector<unsigned long long> &meta, std::vector<uint64_t> &sl,
                        std::vector<uint32_t> &ends, qt_args &T) {
    cq_big_slices(meta, F, sl, ends);
    T.n_slices = (uint32_t)sl.size() - 1;
    T.g_bm = W.surv; T.g_rank = W.surv + (size_t)F.NT * 512; T.g_tcount = T.g_rank + (size_t)F.NT * 512; T.g_nid = T.g_tcount + F.NT;
    uint32_t *d_ends = T.g_nid + F.cap;
    T.g_eend = d_ends; T.g_nend = d_ends + F.big_wpr;
    uint64_t *d_sl = (uint64_t *)(((uintptr_t)(d_ends + 2 * F.big_wpr) + 63) & ~(uintptr_t)63);
    T.slices = d_sl;
    T.partial = W.partial; T.g_rowbits = W.rowbits; T.g_wpr = F.big_wpr;
    (void)hipMemcpyAsync(d_ends, ends.data(), ends.size() * 4, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(d_sl, sl.data(), sl.size() * 8, hipMemcpyHostToDevice, c->stream);
}

// plan (list positions, CQ_SEG-byte segments) + segment-parallel scoring of the query hashes in A (k_query.hip)
static int cq_score(fdgpu_ctx *c, const cq_args &A, const cq_scratch &W, int64_t known_segments) {
    hipStream_t st = c->stream;
    fd_launch_cq_plan(A, W.kidx, W.nseg, st);
    fd_exclusive_scan<uint32_t>(W.nseg, A.nq, W.wstart, W.scan_tmp, W.total, st);
    HIPCHK(c, hipGetLastError());
    uint64_t n_seg = (uint64_t)known_segments;      // the caller knows the work count (query maps remember their hashes' segments): no round trip
    if (known_segments < 0) {
        int rc = d2h_u64(c, W.total, &n_seg);
        if (rc) return rc;
    }
    HIPCHK(c, c->ws[WS_CQ_SEGSUM].ensure(std::max<uint64_t>(n_seg, 1) * 4));       // (sized by the work count: not in cq_reserve)
    fd_launch_cq_seg(A, W.kidx, W.wstart, c->ws[WS_CQ_SEGSUM].as<uint32_t>(), n_seg, n_seg > 0, st);
    return FDGPU_OK;
}
// The rows form: occupancy rows, then per (query, structure) the counts from them and the scan of the touched flags that places the compaction's records.
// Thousands of rows (whole-structure queries): S / 4096 workgroups of word columns do not fill the chip — the rows are cut into ~32 slices at node
// boundaries.  slices: the caller's, it outlives its asynchronous copy (every path synchronises the stream before it returns).
static int cq_score_rows(fdgpu_ctx *c, const cq_args &A, const cq_form &F, const cq_scratch &W, const cq_inputs &In, const std::vector<unsigned long long> &meta,
                         uint64_t n_queries, int64_t known_segments, std::vector<uint64_t> &slices) {
    hipStream_t st = c->stream;
    StageTimer t(c, "cq_batch", 0);
    int rs = cq_score(c, A, W, known_segments);
    if (rs) return rs;
    if (F.sliced) {
        const uint64_t nq = A.nq, per = (nq + 31) / 32;
        slices.push_back(0);
        for (uint64_t r = 0; r + 1 < nq; ++r)
            if ((meta[r] & 2ull) && r + 1 - slices.back() >= per) slices.push_back(r + 1);
        slices.push_back(nq);
        if (hipMemcpyAsync(W.slices, slices.data(), slices.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess) slices.clear();
    }
    if (!F.keys_only)
        fd_launch_cq_rows_finalize(A, In.q_off, (uint32_t)n_queries, slices.empty() ? nullptr : W.slices, slices.empty() ? 0u : (uint32_t)slices.size() - 1,
                                   W.node_cnt, W.edge_cnt, W.flags, F.max_rows, st);
    if (!F.dense_topn) fd_exclusive_scan<uint8_t>(W.flags, F.QS, W.pos, W.scan_tmp, W.total, st);
    return FDGPU_OK;
}
static void cq_score_tiled(fdgpu_ctx *c, const cq_args &A, const qt_args &T, const cq_form &F, const cq_scratch &W, const cq_inputs &In) {
    hipStream_t st = c->stream;
    StageTimer t(c, "cq_batch", 0);
    if (!In.have_k) fd_launch_cq_plan(A, In.kidx, W.nseg, st);
    if (F.qt32) { fd_launch_qt_layout(T, st); fd_launch_qt_score32(T, st); }
    else { fd_launch_qt_plan(T, st); if (F.tiled_big) fd_launch_qt_big_score(T, st); else fd_launch_qt_score(T, st); }
}

// Candidate selection straight from the scores (k_qt_select, or k_topn_*_dense + k_topn_sort on the rows form's dense results): no flag scan, no
// compaction of every touched structure, one synchronisation instead of three.  dev != null: the ranked selection stays on the device (see
// fd_count_query_batch_impl).  *overflow: more ties at a cut-off than the selection's slots hold — nothing is returned, the compacting path ranks that call.
static int cq_select_on_device(fdgpu_ctx *c, const cq_form &F, const cq_scratch &W, const cq_args &A, const qt_args &T, const cq_inputs &In, uint64_t n_queries,
                               uint32_t top_n, fd_cq_dev_out *dev, const cq_stamps &stamps, cq_off_ptr &ooff, fd_count_rec **out, uint64_t **out_off, bool *overflow) {
    hipStream_t st = c->stream;
    std::vector<uint32_t> tstate((size_t)n_queries * 4);
    // the ranked records land in the caller's array (page-locked, pooled) at a stride of top_n and are closed up in place afterwards
    cq_pooled_ptr rr(dev ? nullptr : (fd_count_rec *)fd_out_alloc(std::max<uint64_t>((uint64_t)n_queries * top_n, 1) * sizeof(fd_count_rec), true));
    if (!dev && !rr) return FDGPU_ENOMEM;
    {
        StageTimer t(c, "cq_topn", 0);
        if (F.tiled) fd_launch_qt_select(T, top_n, W.ranked, st);
        else if (F.tiled_big) fd_launch_qt_big_select(T, top_n, W.ranked, st);
        else {
            if (F.keys_only) fd_launch_cq_topn_dense(A, In.q_off, In.penalty, W.keys, (uint32_t)n_queries, top_n, F.cap, W.sel, W.sel_state, W.ghist, st);
            else fd_launch_cq_topn_acc(A, In.penalty, W.node_cnt, W.edge_cnt, (uint32_t)n_queries, top_n, F.cap, W.sel, W.sel_state, W.ghist, st);
            fd_launch_cq_topn_sort(W.sel, F.cap, W.sel_state, (uint32_t)n_queries, top_n, W.ranked, st);
        }
    }
    if (stamps.on) fprintf(stderr, "[count_query] launched at %.3f ms\n", stamps.ms());
    if (dev && dev->while_running && *dev->while_running) (*dev->while_running)();
    hipError_t e = hipMemcpyAsync(tstate.data(), W.sel_state, n_queries * 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !dev) e = hipMemcpyAsync(rr.get(), W.ranked, (size_t)n_queries * top_n * sizeof(fd_count_rec), hipMemcpyDeviceToHost, st);
    fd_count_rec *head = nullptr;      // the caller's candidates (fdgpu_query_batch: match_top per query) ride on the same wait
    if (e == hipSuccess && dev && dev->head_n) {
        const uint32_t mt = std::min(dev->head_n, top_n);
        head = (fd_count_rec *)c->host_pinned(FD_HP_UP, (size_t)n_queries * mt * sizeof(fd_count_rec));
        if (head) e = hipMemcpy2DAsync(head, (size_t)mt * sizeof(fd_count_rec), W.ranked, (size_t)top_n * sizeof(fd_count_rec), (size_t)mt * sizeof(fd_count_rec), n_queries,
                                       hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("count_query_batch: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    if (stamps.on) fprintf(stderr, "[count_query] records on the host at %.3f ms\n", stamps.ms());
    for (uint64_t t = 0; t < n_queries; ++t) *overflow = *overflow || tstate[4 * t + 3] > F.cap;
    if (dev) {        // the ranked selection stays where it is
        dev->counts.resize(n_queries);
        for (uint64_t t = 0; t < n_queries; ++t) dev->counts[t] = tstate[4 * t + 3];
        dev->head = head;
        dev->got = true; dev->overflow = *overflow; dev->recs = W.ranked; dev->state = W.sel_state; dev->top_n = top_n; dev->cap = F.cap;
        *overflow = false;      // (the caller's to handle, together with the other ranks)
        return FDGPU_OK;
    }
    if (*overflow) return FDGPU_OK;
    uint64_t w = 0;
    for (uint64_t t = 0; t < n_queries; ++t) {
        const uint64_t m = std::min<uint32_t>(tstate[4 * t + 3], top_n);
        ooff.get()[t] = w;
        if (m && w != t * top_n) memmove(rr.get() + w, rr.get() + (size_t)t * top_n, (size_t)m * sizeof(fd_count_rec));      // w <= t * top_n: forward
        w += m;
    }
    ooff.get()[n_queries] = w;
    *out = rr.release(); *out_off = ooff.release();
    return FDGPU_OK;
}

// Per-query preselection of the top_n by idf among the compacted records (k_cq_topn); a query whose threshold bin overflows the fixed-stride output falls
// back to its full list.  In: ooff = the queries' first compacted records; out: the ranked records and their offsets.
static int cq_select_compacted(fdgpu_ctx *c, cq_scratch &W, uint64_t n_queries, uint32_t top_n, cq_off_ptr &ooff, fd_count_rec **out, uint64_t **out_off) {
    hipStream_t st = c->stream;
    const uint32_t cap = top_n + 1024;
    const bool dev_sort = cap <= 4096;          // k_topn_sort ranks and cuts on the device: only top_n records per query cross the bus
    const uint32_t stride = dev_sort ? top_n : cap;
    std::vector<fd_count_rec> sel((size_t)n_queries * stride);
    std::vector<uint32_t> tstate((size_t)n_queries * 4);
    hipError_t e = cq_reserve_selection(c, n_queries, top_n, cap, dev_sort ? WS_KEYS_B : -1, W);
    if (e == hipSuccess) {
        fd_launch_cq_topn(W.records, W.rec_off, (uint32_t)n_queries, top_n, cap, W.sel, W.sel_state, W.ghist, st);
        if (dev_sort) fd_launch_cq_topn_sort(W.sel, cap, W.sel_state, (uint32_t)n_queries, top_n, W.ranked, st);
        e = hipMemcpyAsync(tstate.data(), W.sel_state, n_queries * 16, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(sel.data(), dev_sort ? W.ranked : W.sel, sel.size() * sizeof(fd_count_rec), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("count_query_batch: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    uint64_t *const off = ooff.get();
    auto kept = [&](uint64_t t) -> uint64_t { return dev_sort ? std::min<uint32_t>(tstate[4 * t + 3], top_n) : tstate[4 * t + 3]; };
    uint64_t tot = 0;
    for (uint64_t t = 0; t < n_queries; ++t) tot += tstate[4 * t + 3] <= cap ? kept(t) : off[t + 1] - off[t];
    cq_rec_ptr r((fd_count_rec *)malloc(std::max<uint64_t>(tot, 1) * sizeof(fd_count_rec)));
    if (!r) return FDGPU_ENOMEM;
    std::vector<uint64_t> noff(n_queries + 1, 0);
    for (uint64_t t = 0; t < n_queries; ++t) {
        fd_count_rec *const dst = r.get() + noff[t];
        uint64_t m = kept(t);
        if (tstate[4 * t + 3] <= cap) {
            memcpy(dst, sel.data() + (size_t)t * stride, (size_t)m * sizeof(fd_count_rec));
            if (!dev_sort) m = fd_rank_trim(dst, m, top_n);
        } else {
            m = off[t + 1] - off[t];
            if (hipMemcpy(dst, (const fd_count_rec *)W.records + off[t], m * sizeof(fd_count_rec), hipMemcpyDeviceToHost) != hipSuccess)
                FAIL(c, FDGPU_EHIP, "count_query_batch: fallback copy failed");
            m = fd_rank_trim(dst, m, top_n);
        }
        noff[t + 1] = noff[t] + m;
    }
    memcpy(off, noff.data(), (n_queries + 1) * 8);
    *out = r.release(); *out_off = ooff.release();
    return FDGPU_OK;
}
// The compacting tail of the rows form: every touched (query, structure) as a record in ascending id, the queries' first records read from the flag scan
// at t x S; with top_n the records are cut on the device when there are many, on the host when there are few.
static int cq_compact_home(fdgpu_ctx *c, const cq_form &F, cq_scratch &W, const cq_args &A, const cq_inputs &In, uint64_t n_queries, uint32_t top_n,
                           cq_off_ptr &ooff, fd_count_rec **out, uint64_t **out_off) {
    hipStream_t st = c->stream;
    uint64_t n = 0;
    int rc = d2h_u64(c, W.total, &n);
    if (rc) return rc;
    const bool select = top_n > 0 && n > (uint64_t)top_n * n_queries;   // worth preselecting on the device
    cq_rec_ptr r(select ? nullptr : (fd_count_rec *)malloc(std::max<uint64_t>(n, 1) * sizeof(fd_count_rec)));
    if (!select && !r) return FDGPU_ENOMEM;
    uint64_t *const off = ooff.get();
    std::vector<uint64_t> idx(n_queries + 1);       // must outlive its copy: synchronised below
    for (uint64_t t = 0; t <= n_queries; ++t) idx[t] = t * A.S;
    hipError_t e = cq_reserve_records(c, n, W);
    if (e == hipSuccess) {
        fd_launch_cq_compact_batch(A, W.node_cnt, W.edge_cnt, W.flags, W.pos, In.penalty, F.QS, W.records, st);
        e = hipMemcpyAsync(W.gather_idx, idx.data(), (n_queries + 1) * 8, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) {
        fd_launch_gather_u64(W.pos, W.gather_idx, n_queries + 1, W.rec_off, st);
        e = hipMemcpyAsync(off, W.rec_off, (n_queries + 1) * 8, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess && select && (e = hipStreamSynchronize(st)) == hipSuccess) return cq_select_compacted(c, W, n_queries, top_n, ooff, out, out_off);
    if (e == hipSuccess && n) e = hipMemcpyAsync(r.get(), W.records, n * sizeof(fd_count_rec), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("count_query_batch: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    if (top_n > 0) {     // few records: ranked and cut on the host, same contract as the device selection
        uint64_t w = 0;
        for (uint64_t t = 0; t < n_queries; ++t) {
            const uint64_t a = off[t], m = fd_rank_trim(r.get() + a, off[t + 1] - a, top_n);
            if (w != a) memmove(r.get() + w, r.get() + a, m * sizeof(fd_count_rec));
            off[t] = w; w += m;
        }
        off[n_queries] = w;
    }
    *out = r.release(); *out_off = ooff.release();
    return FDGPU_OK;
}

// batched count_query: queries [q_off[t], q_off[t+1]) of the concatenated hash arrays; results of query t are (*out)[(*out_off)[t] .. (*out_off)[t+1])
// dev != null: a call whose candidate selection runs on the device (cq_form.dense_topn) leaves its result THERE — dev->recs = [n_queries][top_n]
// ranked records, dev->state = the per-query selection state (count = records selected) — and returns without host records (dev->got); the
// sharded query all-gathers those buffers (fd_comm.hip).  dev->overflow: more ties at a cut-off than the selection holds (the caller
// takes the compacting path together with the other ranks).  Calls the device selection does not serve return host records as usual.
int fd_count_query_batch_impl(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t n_queries, const uint64_t *q_off, const uint32_t *q_hash,
                              const uint32_t *q_node, const uint32_t *q_edge_j, const float *q_idf, const float *penalty, uint32_t top_n,
                              fd_count_rec **out, uint64_t **out_off, bool allow_dense, fd_cq_dev_out *dev, int64_t known_segments, const long long *known_kidx,
                              const uint64_t *known_len) {
    if (!c || !ix || !out || !out_off || !q_off || (ix->n_structures && !penalty && !ix->penalty)) return FDGPU_EINVAL;
    *out = nullptr; *out_off = nullptr;
    reset_timings(c);
    c->last_count_path = 0;
    const uint64_t S = ix->n_structures, nq = q_off[n_queries];
    const cq_stamps stamps;
    cq_off_ptr ooff((uint64_t *)calloc(n_queries + 1, 8));
    if (!ooff) return FDGPU_ENOMEM;
    if (dev) { dev->got = false; dev->overflow = false; }
    if (S == 0 || nq == 0 || n_queries == 0) { *out = (fd_count_rec *)malloc(sizeof(fd_count_rec)); if (*out) *out_off = ooff.release(); return *out ? FDGPU_OK : FDGPU_ENOMEM; }
    if (!q_hash || !q_node || !q_edge_j || !q_idf) return FDGPU_EINVAL;
    if (S >= 0xffffffe0ull || n_queries * S >= (1ull << 34)) FAIL(c, FDGPU_ERANGE, "count_query_batch: n_queries x n_structures too large; split the batch");
    cq_rows R;      // (known_len is per input row: only sums of it matter to the form, no permutation needed)
    cq_order_rows(n_queries, q_off, q_hash, q_node, q_edge_j, q_idf, known_kidx, R);
    if (stamps.on) fprintf(stderr, "[count_query] %llu rows of %llu queries in order at %.3f ms\n", (unsigned long long)nq, (unsigned long long)n_queries, stamps.ms());
    cq_form F = cq_choose_form(c, ix, R, n_queries, nq, top_n, allow_dense, known_len);
    cq_scratch W = {};
    int rc = cq_reserve(c, F, n_queries, nq, S, top_n, W);
    if (rc) return rc;
    c->last_count_path = F.path();
    const cq_inputs In = cq_upload(c, ix, F, W, R, n_queries, q_off, penalty, known_kidx && R.kidx.size() == nq);
    const cq_args A = cq_row_args(ix, F, W, In, nq);
    qt_args T = {};
    std::vector<uint64_t> slices;       // host arrays of the launches below: they outlive their asynchronous copies
    std::vector<uint32_t> ends;
    if (F.rows_form()) {
        rc = cq_score_rows(c, A, F, W, In, R.meta, n_queries, known_segments, slices);
        if (rc) return rc;
    } else {
        T = cq_tile_args(ix, F, W, In, nq, n_queries, top_n);
        if (F.tiled) cq_motif_args(c, F, W, n_queries, T);
        else cq_big_args(c, F, W, R.meta, slices, ends, T);
        cq_score_tiled(c, A, T, F, W, In);
    }
    if (!F.dense_topn) return cq_compact_home(c, F, W, A, In, n_queries, top_n, ooff, out, out_off);
    bool overflow = false;
    rc = cq_select_on_device(c, F, W, A, T, In, n_queries, top_n, dev, stamps, ooff, out, out_off, &overflow);
    if (rc || !overflow) return rc;
    // more ties at the cut-off than the selection's slots hold: a second attempt that takes the compacting path ranks that call
    ooff.reset();
    rc = fd_count_query_batch_impl(c, ix, n_queries, q_off, q_hash, q_node, q_edge_j, q_idf, penalty, top_n, out, out_off, false, nullptr, known_segments);
    c->last_count_path = F.path() | FDGPU_PATH_OVERFLOW;
    return rc;
}
extern "C" int fdgpu_count_query_batch(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t n_queries, const uint64_t *q_off, const uint32_t *q_hash,
                                       const uint32_t *q_node, const uint32_t *q_edge_j, const float *q_idf, const float *penalty,
                                       fd_count_rec **out, uint64_t **out_off) { FD_LOCK(c);
    return fd_count_query_batch_impl(c, ix, n_queries, q_off, q_hash, q_node, q_edge_j, q_idf, penalty, 0, out, out_off, true, nullptr);
}
// count_query of one query, every touched structure in ascending id: the batch of one (the rows form, sliced from 4,096 rows)
extern "C" int fdgpu_count_query(fdgpu_ctx *c, const fdgpu_index *ix, const uint32_t *q_hash, const uint32_t *q_node, const uint32_t *q_edge_j,
                                 const float *q_idf, uint64_t nq, const float *penalty, fd_count_rec **out, uint64_t *n_out) { FD_LOCK(c);
    if (!c || !ix || !out || !n_out || (nq && (!q_hash || !q_node || !q_edge_j || !q_idf)) || (ix->n_structures && !penalty && !ix->penalty)) return FDGPU_EINVAL;
    *out = nullptr; *n_out = 0;
    if (nq && ix->n_structures >= 0xffffffe0ull) FAIL(c, FDGPU_ERANGE, "too many structures");
    const uint64_t q_off[2] = {0, nq};
    uint64_t *off = nullptr;
    const int rc = fd_count_query_batch_impl(c, ix, 1, q_off, q_hash, q_node, q_edge_j, q_idf, penalty, 0, out, &off, true, nullptr);
    const cq_off_ptr owned(off);
    if (rc == FDGPU_OK) *n_out = off[1];
    return rc;
}
// as fdgpu_count_query_batch, but per query only the top_n records come back, RANKED as the candidate selection of query_pdb.rs:404-411 ranks them (idf
// descending, ties by ascending structure id): radix selection + LDS bitonic sort on the device, top_n records per query over the bus
extern "C" int fdgpu_count_query_batch_top(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t n_queries, const uint64_t *q_off, const uint32_t *q_hash,
                                           const uint32_t *q_node, const uint32_t *q_edge_j, const float *q_idf, const float *penalty,
                                           uint32_t top_n, fd_count_rec **out, uint64_t **out_off) { FD_LOCK(c);
    return fd_count_query_batch_impl(c, ix, n_queries, q_off, q_hash, q_node, q_edge_j, q_idf, penalty, top_n, out, out_off, true, nullptr);
}

extern "C" int fdgpu_debug_last_count_path(fdgpu_ctx *c, uint32_t *flags) { FD_LOCK(c);
    if (!c || !flags) return FDGPU_EINVAL;
    *flags = c->last_count_path;
    return FDGPU_OK;
}

// The length penalty nres^(-lp) of the index's structures (count_query.rs:200), kept on the device: count queries may then pass
// penalty = NULL instead of uploading S floats per call.  penalty = NULL drops the resident copy.
extern "C" int fdgpu_index_set_penalty(fdgpu_ctx *c, fdgpu_index *ix, const float *penalty) { FD_LOCK(c);
    if (!c || !ix) return FDGPU_EINVAL;
    if (ix->penalty) { (void)hipFree(ix->penalty); ix->penalty = nullptr; }
    if (!penalty || !ix->n_structures) return FDGPU_OK;
    HIPCHK(c, hipMalloc((void **)&ix->penalty, ix->n_structures * 4));
    HIPCHK(c, hipMemcpy(ix->penalty, penalty, ix->n_structures * 4, hipMemcpyHostToDevice));
    return FDGPU_OK;
}

// count_query for the query maps fdgpu_make_query_map[_batch] returned, without a round trip through the caller: the entries of
// every map (hash, (qi, qj)) are scored with idf = log2(total_structures / posting length) of the hash ITSELF (count_query.rs:181-200;
// the idf inside the map belongs to the pair's observed hash and feeds the retrieval's subgraph idf instead); hashes the index does
// not hold are dropped.  Output as fdgpu_count_query_batch_top.
// every map's hash[] (all queries), then every map's primary_hash[]: the 2 * sum(n) hashes whose posting lengths a sharded query needs
// over the WHOLE database
uint64_t fd_maps_hashes(uint64_t n_queries, const fd_query_map *const *qms, std::vector<uint32_t> &h) {
    uint64_t nq = 0;
    for (uint64_t t = 0; t < n_queries; ++t) nq += qms[t]->n;
    h.assign(std::max<uint64_t>(2 * nq, 1), 0);
    uint64_t at = 0;
    for (uint64_t t = 0; t < n_queries; ++t) { if (qms[t]->n) memcpy(&h[at], qms[t]->hash, qms[t]->n * 4); at += qms[t]->n; }
    for (uint64_t t = 0; t < n_queries; ++t) { if (qms[t]->n) memcpy(&h[at], qms[t]->primary_hash, qms[t]->n * 4); at += qms[t]->n; }
    return nq;
}
// scoring of query maps with the posting lengths given: len[0 .. nq) belong to the maps' hash[] in order (idf = log2f(total / len), absent
// hashes drop out); with primary_len the maps' own idf[] (the retrieval's subgraph idf, query.rs:283-288) is rewritten from the lengths
// of primary_hash[] — what a sharded index needs, whose make_query_map saw one shard only
int fd_count_query_maps_len(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t n_queries, const fd_query_map *const *qms, const uint64_t *len,
                            const uint64_t *primary_len, const float *penalty, float total_structures, uint32_t top_n, fd_count_rec **out,
                            uint64_t **out_off, fd_cq_dev_out *dev, const uint32_t *seg, const long long *kidx, bool allow_dense) {
    uint64_t nq = 0;
    int64_t W = seg ? 0 : -1;
    for (uint64_t t = 0; t < n_queries; ++t) nq += qms[t]->n;
    std::vector<uint64_t> q_off(n_queries + 1, 0);
    std::vector<uint32_t> qh, qn, qe;
    std::vector<float> qi;
    std::vector<long long> qk;
    std::vector<uint64_t> ql;       // the kept rows' posting lengths (local to this index only when the lengths are: the tiled path sizes its stream from them)
    // (filled through plain pointers: a whole-structure query is 10^5 rows, six push_backs each were a third of this loop)
    qh.resize(nq + 1); qn.resize(nq + 1); qe.resize(nq + 1); qi.resize(nq + 1); ql.resize(nq + 1);
    if (kidx) qk.resize(nq + 1);
    uint32_t *const p_h = qh.data(), *const p_n = qn.data(), *const p_e = qe.data();
    float *const p_i = qi.data();
    uint64_t *const p_l = ql.data();
    long long *const p_k = kidx ? qk.data() : nullptr;
    uint64_t at = 0, w = 0;
    for (uint64_t t = 0; t < n_queries; ++t) {
        const fd_query_map *m = qms[t];
        const uint32_t *const mh = m->hash, *const mqi = m->qi, *const mqj = m->qj;
        float *const midf = m->idf;
        const uint64_t mn = m->n;
        for (uint64_t k = 0; k < mn; ++k, ++at) {
            if (primary_len) midf[k] = primary_len[at] ? log2f(total_structures / (float)primary_len[at]) : 0.0f;
            const uint64_t L = len[at];
            if (!L) continue;
            p_h[w] = mh[k]; p_n[w] = mqi[k]; p_e[w] = mqj[k];
            if (p_k) p_k[w] = kidx[at];
            p_l[w] = L;
            if (seg) W += seg[at];
            ++w;
        }
        q_off[t + 1] = w;
    }
    // idf of the kept rows: f32 like the reference's (total / len).log2().  log2f is ~8 ns a call: the 10^5 rows of a whole-structure query in eight parts on
    // the context's helper threads (0.6 ms of the call's host time on one)
    auto idf_rows = [&](uint64_t a, uint64_t b) { for (uint64_t r = a; r < b; ++r) p_i[r] = log2f(total_structures / (float)p_l[r]); };
    if (w < 16384) idf_rows(0, w);
    else {
        const unsigned nt = 8;
        std::atomic<unsigned> part(0);
        const std::function<void()> wk = [&]() { for (;;) { const unsigned k = part.fetch_add(1); if (k >= nt) break; idf_rows(w * k / nt, w * (k + 1) / nt); } };
        c->host_pool.run(c->small_par(nt), wk);
    }
    qh.resize(w); qn.resize(w); qe.resize(w); qi.resize(w); ql.resize(w);
    if (kidx) qk.resize(w);
    if (qh.empty()) { qh.push_back(0); qn.push_back(0); qe.push_back(0); qi.push_back(0.0f); W = seg ? 0 : -1; qk.clear(); ql.clear(); }
    // (the lengths bound the LOCAL lists only when they are this index's own: the caller that passes kidx made the maps against it)
    return fd_count_query_batch_impl(c, ix, n_queries, q_off.data(), qh.data(), qn.data(), qe.data(), qi.data(), penalty, top_n, out, out_off, allow_dense, dev, W,
                                     kidx && qk.size() == qh.size() ? qk.data() : nullptr, kidx && ql.size() == qh.size() ? ql.data() : nullptr);
}
extern "C" int fdgpu_count_query_maps_top(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t n_queries, const fd_query_map *const *qms, const float *penalty,
                                          float total_structures, uint32_t top_n, fd_count_rec **out, uint64_t **out_off) { FD_LOCK(c);
    return fd_count_query_maps_top_impl(c, ix, n_queries, qms, penalty, total_structures, top_n, out, out_off, nullptr);
}
int fd_count_query_maps_top_impl(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t n_queries, const fd_query_map *const *qms, const float *penalty, float total_structures,
                                 uint32_t top_n, fd_count_rec **out, uint64_t **out_off, fd_cq_dev_out *dev, bool allow_dense) { FD_LOCK(c);
    if (!c || !ix || !out || !out_off || (n_queries && !qms)) return FDGPU_EINVAL;
    uint64_t nq = 0;
    for (uint64_t t = 0; t < n_queries; ++t) { if (!qms[t]) return FDGPU_EINVAL; nq += qms[t]->n; }
    std::vector<uint32_t> h(std::max<uint64_t>(nq, 1));
    std::vector<uint64_t> len(std::max<uint64_t>(nq, 1), 0);
    std::vector<uint32_t> seg(std::max<uint64_t>(nq, 1), 0);
    std::vector<long long> kidx(std::max<uint64_t>(nq, 1), -1);
    bool remembered = nq > 0;       // maps made against THIS index carry their hashes' posting lengths, segment counts and list positions
    for (uint64_t t = 0; t < n_queries; ++t) remembered = remembered && (!qms[t]->n || (qms[t]->post_len && qms[t]->post_seg && qms[t]->post_index_uid == ix->uid));
    bool have_kidx = remembered;
    for (uint64_t t = 0; t < n_queries; ++t) have_kidx = have_kidx && (!qms[t]->n || qms[t]->post_kidx);
    uint64_t at = 0;
    for (uint64_t t = 0; t < n_queries; ++t) {
        if (qms[t]->n) {
            if (have_kidx) memcpy(&kidx[at], qms[t]->post_kidx, qms[t]->n * 8);
            if (remembered) { memcpy(&len[at], qms[t]->post_len, qms[t]->n * 8); memcpy(&seg[at], qms[t]->post_seg, qms[t]->n * 4); }
            else memcpy(&h[at], qms[t]->hash, qms[t]->n * 4);
        }
        at += qms[t]->n;
    }
    int rc = !remembered && nq && ix->n_structures ? fd_posting_lengths_segs(c, ix, h.data(), nq, len.data(), seg.data()) : FDGPU_OK;
    if (rc) return rc;
    return fd_count_query_maps_len(c, ix, n_queries, qms, len.data(), nullptr, penalty, total_structures, top_n, out, out_off, dev, seg.data(),
                                   have_kidx ? kidx.data() : nullptr, allow_dense);
}
// The two halves of the sharded form for hosts that bring their own transport (MPI, gloo, ...): the LOCAL posting lengths of the maps'
// hash[] and primary_hash[] (2 * sum(n) values, fd_maps_hashes order) — the caller sums them over the ranks — and the scoring of the
// local shard with those GLOBAL lengths (maps' idf[] rewritten from the primary lengths).  With RCCL: fdgpu_sharded_count_query_maps.
extern "C" int fdgpu_query_maps_lengths(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t n_queries, const fd_query_map *const *qms, uint64_t *lengths) { FD_LOCK(c);
    if (!c || !ix || (n_queries && !qms) || !lengths) return FDGPU_EINVAL;
    for (uint64_t t = 0; t < n_queries; ++t) if (!qms[t]) return FDGPU_EINVAL;
    std::vector<uint32_t> h;
    const uint64_t nq = fd_maps_hashes(n_queries, qms, h);
    return nq ? fdgpu_posting_lengths(c, ix, h.data(), 2 * nq, lengths) : FDGPU_OK;
}
extern "C" int fdgpu_count_query_maps_top_global(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t n_queries, fd_query_map *const *qms, const uint64_t *global_lengths,
                                                 const float *penalty, float total_structures, uint32_t top_n, fd_count_rec **out, uint64_t **out_off) { FD_LOCK(c);
    if (!c || !ix || !out || !out_off || (n_queries && !qms)) return FDGPU_EINVAL;
    uint64_t nq = 0;
    for (uint64_t t = 0; t < n_queries; ++t) { if (!qms[t]) return FDGPU_EINVAL; nq += qms[t]->n; }
    if (nq && !global_lengths) return FDGPU_EINVAL;
    const uint64_t zero = 0;
    return fd_count_query_maps_len(c, ix, n_queries, qms, nq ? global_lengths : &zero, nq ? global_lengths + nq : nullptr, penalty, total_structures, top_n,
                                   out, out_off, nullptr);
}

