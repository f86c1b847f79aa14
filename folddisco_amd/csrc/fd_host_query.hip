// fd_host_query.hip — the retrieval's dispatcher around the GPU kernels, and the fused query call:
//   retrieval             (src/controller/retrieve.rs:364-552)                pair scan + Kabsch on the GPU,
//                          graph components (src/controller/graph.rs:16-50), residue voting
//                          (retrieve.rs:604-702) and rescue (:479-515) on the device for motif queries (rs_*: the device glue's steps), on host
//                          threads for > 64-node queries (rb_*: the host path's stages; the per-slot work itself is fd_retrieve_host.cpp)
//   fdgpu_query_batch      query maps (fd_query_map.hip), ranked scoring and retrieval of the top candidates in one call
//   fdgpu_merge_subindices, fdgpu_hypergeom_enrichment
// The reference is compiled code, so this glue is C++ behind the same C ABI; it contains no f32 arithmetic that decides a hash bit.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>
#include "fd_api_common.h"
#include "fd_postings.h"

extern "C" void fdgpu_matches_free(fd_match_rec *m, int32_t *residues) { fdgpu_free(m); fdgpu_free(residues); }

// coordinates of all candidates in one launch + one copy (a hipMemcpy per candidate costs more than the pair scan)
__global__ __launch_bounds__(256) void k_gather_xyz(const float *__restrict__ ca, const float *__restrict__ cb, const uint64_t *__restrict__ src,
                                                    const uint64_t *__restrict__ dst, uint64_t total, float *__restrict__ out) {
    const uint64_t k = blockIdx.x;
    const uint64_t s3 = 3 * src[k], d3 = 3 * dst[k], n3 = 3 * (dst[k + 1] - dst[k]);
    for (uint64_t t = threadIdx.x; t < n3; t += blockDim.x) {
        out[d3 + t] = ca[s3 + t];
        out[3 * total + d3 + t] = cb[s3 + t];
    }
}

namespace {
typedef std::chrono::steady_clock::time_point rb_time;
inline rb_time t_now() { return std::chrono::steady_clock::now(); }
inline double t_ms(rb_time a, rb_time b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// a retrieval call's arguments as every stage reads them (prep: the maps' tables, the caller's or the call's own)
struct rb_in {
    fdgpu_ctx *c; const fdgpu_batch *db; const uint8_t *resname_std; uint64_t n_queries; const uint32_t *cand; const uint64_t *cand_off;
    const fd_query_map *const *qms; const fdgpu_batch *qb; const uint32_t *q_struct; const fd_hash_params *p; uint32_t node_count, partial_fit;
    uint64_t n_cand; const fd_rb_prep *prep; bool trace; rb_time T0;
};
struct rb_out { fd_match_rec **matches; uint64_t **match_off; int32_t **residues; uint64_t **res_off; };
// result arrays on their way out: freed here unless released into the caller's pointers (fdgpu_free takes pooled and malloc'ed blocks alike)
template <typename T> struct rb_owned {
    T *p = nullptr;
    explicit rb_owned(T *q) : p(q) {}
    rb_owned(const rb_owned &) = delete;
    ~rb_owned() { fdgpu_free(p); }
    T *release() { T *q = p; p = nullptr; return q; }
};
}  // namespace

// ---- device glue (k_retrieve.hip): the scan output never leaves the GPU — per-slot grouping, graph / components / votes /
// assignment / rescue one wavefront per candidate, superposition and metrics on the problems it wrote, then ONE copy of the match
// records back.  Taken for motif-sized queries (<= 64 query residues, single scan, no --partial-fit); a candidate beyond the
// kernel's limits (64 graph nodes, 1024 found triples) raises a flag and the whole call takes the host path below instead.
namespace {
// the glue's tables as one packed block of 32-bit words: where each table starts, the block's size, the block (a pinned staging buffer of the
// context, or own when there is none)
struct rs_layout {
    size_t o_qt = 0, o_h = 0, o_kf = 0, o_sy = 0, o_qi = 0, o_qj = 0, o_idf = 0, o_idx = 0, o_sq = 0, o_cd = 0, o_d0 = 0, o_co = 0, words = 0;
    uint32_t *blk = nullptr;
};
// what the reserve step fixes for the launches: capacities, the scan's record counts, the grouping's arrays, the ordering block, the kernels' arguments
struct rs_plan {
    uint64_t nf_d = 0, nc_d = 0, cap_m = 0, cap_prob = 0, cap_res = 0, cap_pts = 0;
    size_t cnt_bytes = 0;                                              // the counters, the slots' record counts, the grouping's counts: zeroed by one fill
    uint32_t *d_cnt = nullptr, *d_seg = nullptr, *d_cur = nullptr, *d_pf = nullptr, *d_pc = nullptr;
    uint32_t *d_ord = nullptr; size_t o_scr = 0, o_mo = 0, o_ro = 0;   // [slot bases + first residues (2 n_cand + 2) | match_off, res_off (n_queries + 1 each, 8-byte)] for the device-side ordering
    rs_args A;
};
}  // namespace

// tables: one packed host block -> one copy.  Built WHILE the pair scan runs (it needs none of the scan's output): the scan's launch
// is followed by ~0.4 ms of kernel per 128 queries that the host used to wait out before starting on this
static rs_layout rs_pack_tables(const rb_in &I, std::vector<uint32_t> &blk_own) {
    const uint64_t n_queries = I.n_queries, n_cand = I.n_cand;
    const std::vector<std::vector<uint32_t>> &qhs = I.prep->qhs, &qkf = I.prep->qkf;
    const uint32_t htype = I.p->hash_type;
    std::vector<rs_query_dev> qt(n_queries);
    std::vector<uint32_t> t_hash, t_kfirst, t_sym, t_qi, t_qj, t_idf, t_idx;
    {
        size_t th = 0, tm = 0, ti = 0;
        for (uint64_t t = 0; t < n_queries; ++t) { th += qhs[t].size(); tm += I.qms[t]->n; ti += I.qms[t]->n_indices; }
        t_hash.reserve(th); t_kfirst.reserve(th); t_sym.reserve(th); t_qi.reserve(tm); t_qj.reserve(tm); t_idf.reserve(tm); t_idx.reserve(ti);
    }
    for (uint64_t t = 0; t < n_queries; ++t) {
        const fd_query_map *m = I.qms[t];
        rs_query_dev &Q = qt[t];
        memset(&Q, 0, sizeof Q);
        Q.qh_off = (uint32_t)t_hash.size(); Q.n_hashes = (uint32_t)qhs[t].size();
        t_hash.insert(t_hash.end(), qhs[t].begin(), qhs[t].end());
        t_kfirst.insert(t_kfirst.end(), qkf[t].begin(), qkf[t].end());
        for (size_t z = 0; z < qhs[t].size(); ++z) t_sym.push_back(fd_hash_is_sym(htype, qhs[t][z]) ? 1u : 0u);
        Q.map_off = (uint32_t)t_qi.size();
        t_qi.insert(t_qi.end(), m->qi, m->qi + m->n);
        t_qj.insert(t_qj.end(), m->qj, m->qj + m->n);
        t_idf.resize(t_idf.size() + m->n);
        if (m->n) memcpy(t_idf.data() + t_idf.size() - m->n, m->idf, m->n * 4);
        Q.idx_off = (uint32_t)t_idx.size(); Q.n_idx = (uint32_t)m->n_indices;
        t_idx.insert(t_idx.end(), m->indices, m->indices + m->n_indices);
        Q.q_size = I.prep->q_sizes[t];
        Q.q_res0 = (uint32_t)I.qb->h_res_off[I.q_struct[t]];
    }
    std::vector<uint32_t> t_slotq(n_cand);
    for (uint64_t t = 0; t < n_queries; ++t) for (uint64_t k = I.cand_off[t]; k < I.cand_off[t + 1]; ++k) t_slotq[k] = (uint32_t)t;
    float d0tab[2 * FD_WAVE + 1];
    for (int len = 0; len <= 2 * FD_WAVE; ++len) d0tab[len] = len > 21 ? 1.24f * powf((float)len - 15.0f, 1.0f / 3.0f) - 1.8f : 0.5f;   // metrics.rs:117-123
    auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    const size_t nh = t_hash.size(), nmap = t_qi.size(), nidx = t_idx.size();
    rs_layout L;
    L.o_qt = 0; L.o_h = L.o_qt + up4(n_queries * (sizeof(rs_query_dev) / 4)); L.o_kf = L.o_h + up4(nh); L.o_sy = L.o_kf + up4(nh); L.o_qi = L.o_sy + up4((nh + 3) / 4);
    L.o_qj = L.o_qi + up4(nmap); L.o_idf = L.o_qj + up4(nmap); L.o_idx = L.o_idf + up4(nmap); L.o_sq = L.o_idx + up4(nidx); L.o_cd = L.o_sq + up4(n_cand);
    L.o_d0 = L.o_cd + up4(n_cand); L.o_co = L.o_d0 + up4(2 * FD_WAVE + 1); L.words = L.o_co + up4(2 * (n_queries + 1)) + 4;
    // packed in a pinned staging buffer of the context (its own: the pair scan's block in FD_HP_SCAN_A is being copied while this runs)
    uint32_t *blk = (uint32_t *)I.c->host_pinned(FD_HP_LAND, L.words * 4);
    if (!blk) { blk_own.assign(L.words, 0); blk = blk_own.data(); }
    memcpy(&blk[L.o_qt], qt.data(), n_queries * sizeof(rs_query_dev));
    if (nh) { memcpy(&blk[L.o_h], t_hash.data(), nh * 4); memcpy(&blk[L.o_kf], t_kfirst.data(), nh * 4); }
    for (size_t k = 0; k < nh; ++k) ((uint8_t *)&blk[L.o_sy])[k] = (uint8_t)t_sym[k];
    if (nmap) { memcpy(&blk[L.o_qi], t_qi.data(), nmap * 4); memcpy(&blk[L.o_qj], t_qj.data(), nmap * 4); memcpy(&blk[L.o_idf], t_idf.data(), nmap * 4); }
    if (nidx) memcpy(&blk[L.o_idx], t_idx.data(), nidx * 4);
    memcpy(&blk[L.o_sq], t_slotq.data(), n_cand * 4);
    memcpy(&blk[L.o_cd], I.cand, n_cand * 4);
    memcpy(&blk[L.o_d0], d0tab, sizeof d0tab);
    memcpy(&blk[L.o_co], I.cand_off, (n_queries + 1) * 8);      // (o_co is a multiple of 4 words: 8-byte aligned)
    L.blk = blk;
    return L;
}

// every workspace of the glue at its size, THEN the pointers into them (an ensure() may move its buffer: none is taken before its slot's last one)
static int rs_reserve(const rb_in &I, const rs_layout &L, rs_plan &R) {
    fdgpu_ctx *c = I.c;
    const uint64_t n_cand = I.n_cand, n_queries = I.n_queries, max_nq = I.prep->max_nq;
    R.cap_m = std::max<uint64_t>(4096, 4 * n_cand); R.cap_prob = 2 * R.cap_m; R.cap_res = R.cap_m * 2 * max_nq;
    R.cap_pts = R.cap_prob * 2 * max_nq;       // a mapping holds at most one target per query residue: <= 2 max_nq [CA, CB] points
    const uint64_t cap_m = R.cap_m, cap_prob = R.cap_prob, cap_pts = R.cap_pts, nf_d = R.nf_d, nc_d = R.nc_d;
    R.cnt_bytes = (2 * RS_CNT_STRIDE + 8) * 8 + (3 * n_cand + 4) * 4;
    R.o_scr = (n_cand + 1) & ~(size_t)1; R.o_mo = (R.o_scr + 2 * n_cand + 2 + 1) & ~(size_t)1; R.o_ro = R.o_mo + 2 * (n_queries + 1);
    const size_t ord_words = R.o_ro + 2 * (n_queries + 1);
    // the split form of the glue (k_rs_setup + a wavefront per component, k_retrieve.hip); FDGPU_RS_SPLIT=0: k_rs_slots alone (read per call: tests compare the two)
    const bool split = !(getenv("FDGPU_RS_SPLIT") && getenv("FDGPU_RS_SPLIT")[0] == '0');
    auto up16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t o_big = 0, o_head = o_big + up16(n_cand * 4), o_nodes = o_head + n_cand * 32, o_comps = o_nodes + n_cand * FD_WAVE * 4,
                 o_work = o_comps + n_cand * 2 * FD_WAVE * 8, o_np = o_work + up16(cap_m * 8), o_gq = o_np + cap_m * 16, o_gr = o_gq + cap_m * 2 * FD_WAVE * 4,
                 o_edges = o_gr + cap_m * 2 * FD_WAVE * 4, sp_bytes = o_edges + (size_t)nf_d * 16 + 16;
    HIPCHK(c, c->ws[WS_RS_TAB].ensure(L.words * 4));
    HIPCHK(c, c->ws[WS_RS_SEG].ensure((6 * (n_cand + 1) + nf_d + nc_d + 4) * 4));
    HIPCHK(c, c->ws[WS_RS_OUT].ensure(cap_m * sizeof(rs_match_dev)));
    HIPCHK(c, c->ws[WS_RS_RES].ensure(R.cap_res * 4));
    HIPCHK(c, c->ws[WS_RS_KX].ensure(cap_pts * 12));
    HIPCHK(c, c->ws[WS_RS_KY].ensure(cap_pts * 12));
    HIPCHK(c, c->ws[WS_RS_GQ].ensure(cap_pts * 4));      // gq | gr: one entry per residue pair (two points) each
    HIPCHK(c, c->ws[WS_RS_KOFF].ensure((cap_prob + 1) * 8 + cap_prob * 4));
    HIPCHK(c, c->ws[WS_RS_SOL].ensure(cap_prob * 18 * 4));
    HIPCHK(c, c->ws[WS_RS_CNT].ensure(R.cnt_bytes));
    HIPCHK(c, c->ws[WS_RS_PLAN].ensure(ord_words * 4));
    if (split) HIPCHK(c, c->ws[WS_RS_SPLIT].ensure(sp_bytes));
    R.d_ord = c->ws[WS_RS_PLAN].as<uint32_t>();
    const uint32_t *dblk = c->ws[WS_RS_TAB].as<uint32_t>();
    uint32_t *sg = c->ws[WS_RS_SEG].as<uint32_t>();
    unsigned long long *counters = c->ws[WS_RS_CNT].as<unsigned long long>();
    R.d_cnt = (uint32_t *)(counters + 2 * RS_CNT_STRIDE + 8) + (n_cand + 2); R.d_seg = sg + 2 * (n_cand + 1); R.d_cur = sg + 4 * (n_cand + 1);
    R.d_pf = sg + 6 * (n_cand + 1); R.d_pc = R.d_pf + nf_d;
    rs_args &A = R.A;
    memset(&A, 0, sizeof A);
    A.found = c->ws[WS_KEYS_A].as<fd_pair_rec>(); A.cands = c->ws[WS_KEYS_B].as<fd_cand_rec>();      // where the scan left its records (mode bit 4)
    A.seg_f = R.d_seg; A.seg_c = R.d_seg + (n_cand + 1); A.perm_f = R.d_pf; A.perm_c = R.d_pc;
    A.cand = dblk + L.o_cd; A.slot_q = dblk + L.o_sq;
    A.slot_matches = (uint32_t *)(counters + 2 * RS_CNT_STRIDE + 8);
    A.order = R.d_cur;      // slots launch heaviest first
    A.db_res_off = I.db->res_off; A.db_ca = I.db->ca_xyz; A.db_cb = I.db->cb_xyz; A.q_ca = I.qb->ca_xyz; A.q_cb = I.qb->cb_xyz;
    A.qt = (const rs_query_dev *)(dblk + L.o_qt); A.hashes = dblk + L.o_h; A.kfirst = dblk + L.o_kf; A.sym = (const uint8_t *)(dblk + L.o_sy);
    A.map_qi = dblk + L.o_qi; A.map_qj = dblk + L.o_qj; A.map_idf = (const float *)(dblk + L.o_idf); A.indices = dblk + L.o_idx;
    A.d0tab = (const float *)(dblk + L.o_d0); A.node_count = I.node_count;
    { const char *nc_env = getenv("FDGPU_RS_NODE_CAP"); const long v = nc_env ? atol(nc_env) : 0; A.node_cap = v > 0 && v < FD_WAVE ? (uint32_t)v : FD_WAVE; }
    A.counters = counters; A.flags = (uint32_t *)(A.counters + 4);
    A.matches = c->ws[WS_RS_OUT].as<rs_match_dev>(); A.residues = c->ws[WS_RS_RES].as<int32_t>();
    A.kx = c->ws[WS_RS_KX].as<float>(); A.ky = c->ws[WS_RS_KY].as<float>();
    A.gq = c->ws[WS_RS_GQ].as<uint32_t>(); A.gr = A.gq + cap_pts / 2;
    A.koff = c->ws[WS_RS_KOFF].as<uint64_t>(); A.d0 = (float *)(A.koff + cap_prob + 1);
    A.cap_matches = cap_m; A.cap_res = R.cap_res; A.cap_prob = cap_prob; A.cap_pts = cap_pts;
    if (split) {
        c->last_retrieve_path |= FDGPU_RPATH_SPLIT;
        uint8_t *sp = c->ws[WS_RS_SPLIT].as<uint8_t>();
        A.sp_big = (uint32_t *)(sp + o_big); A.sp_head = (uint4 *)(sp + o_head); A.sp_nodes = (uint32_t *)(sp + o_nodes);
        A.sp_comps = (unsigned long long *)(sp + o_comps); A.sp_work = (uint2 *)(sp + o_work); A.sp_edges = (uint4 *)(sp + o_edges);
        A.sp_np = (uint4 *)(sp + o_np); A.sp_gq = (uint32_t *)(sp + o_gq); A.sp_gr = (uint32_t *)(sp + o_gr);
        A.sp_big_n = (uint32_t *)(counters + 6);      // zeroed with the counters (flags at + 4)
    }
    return FDGPU_OK;
}

// tables up, counters zeroed, grouping, the slots; then the counters back: cnt_h[0] records, [1] problems << 40 | points, [2] residue ints, [4] flags
static int rs_launch(const rb_in &I, const rs_layout &L, const rs_plan &R, unsigned long long cnt_h[32]) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_RS_TAB].p, L.blk, L.words * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(c->ws[WS_RS_CNT].p, 0, R.cnt_bytes, st));
    fd_launch_rs_group(R.A.found, R.nf_d, R.A.cands, R.nc_d, (uint32_t)I.n_cand, R.d_cnt, R.d_seg, R.d_cur, R.d_pf, R.d_pc, st);
    {
        StageTimer tm(c, "retrieve_slots", 0);
        fd_launch_rs_slots(R.A, (uint32_t)I.n_cand, st);
    }
    HIPCHK(c, hipGetLastError());
    std::vector<unsigned long long> cv(2 * RS_CNT_STRIDE + 8);      // the three counters live 4 KB apart (rs_args.counters)
    HIPCHK(c, hipMemcpyAsync(cv.data(), c->ws[WS_RS_CNT].p, cv.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(cnt_h, cv.data(), 32 * 8);
    cnt_h[1] = cv[RS_CNT_STRIDE]; cnt_h[2] = cv[2 * RS_CNT_STRIDE];
    return FDGPU_OK;
}

// points, Kabsch, metrics on the problems the slots wrote; the records' final places are computed on the device (k_rs_offsets: bases of the slots
// from their record counts; a record's place inside its slot was fixed when it was written) — no header copy, no host sort, no gather plan: after
// the counters nothing but the finished arrays crosses the bus, with one wait
static int rs_finish(const rb_in &I, const rs_layout &L, const rs_plan &R, const unsigned long long cnt_h[32], rb_time D1, rb_time D2, const rb_out &out, fd_rb_dev_out *dev_out) {
    fdgpu_ctx *c = I.c;
    hipStream_t st = c->stream;
    const rs_args &A = R.A;
    const uint64_t n_queries = I.n_queries;
    const uint64_t nm = cnt_h[0], nprob = cnt_h[1] >> 40, npts = cnt_h[1] & ((1ull << 40) - 1ull), tot_res = cnt_h[2];
    if (tot_res >= (1ull << 32)) { c->err = "retrieve_batch: residue lists beyond 2^32 entries; split the batch"; return FDGPU_ERANGE; }
    float *d_rmsd0 = c->ws[WS_RS_SOL].as<float>(), *d_rot0 = d_rmsd0 + nprob, *d_tran0 = d_rot0 + 9 * nprob, *d_met0 = d_tran0 + 3 * nprob;
    rb_owned<uint64_t> omo((uint64_t *)malloc((n_queries + 1) * 8)), oro((uint64_t *)malloc((n_queries + 1) * 8));
    // dev_out: the ordered records stay in the workspaces for the caller (sharded retrieval: gathered device to device); only the offsets return
    rb_owned<fd_match_rec> om(dev_out ? nullptr : (fd_match_rec *)fd_out_alloc(std::max<size_t>(nm, 1) * sizeof(fd_match_rec), true));
    rb_owned<int32_t> orr(dev_out ? nullptr : (int32_t *)fd_out_alloc(std::max<size_t>(tot_res, 1) * sizeof(int32_t), true));
    if (!omo.p || !oro.p || (!dev_out && (!om.p || !orr.p))) return FDGPU_ENOMEM;
    hipError_t e = c->ws[WS_RS_REC].ensure(std::max<uint64_t>(nm, 1) * sizeof(fd_match_rec));
    if (e == hipSuccess) e = c->ws[WS_RS_RECRES].ensure(std::max<uint64_t>(tot_res, 1) * 4);
    if (e == hipSuccess && nprob) {
        fd_launch_rs_points(A, nprob, npts, st);
        fd_launch_kabsch(A.kx, A.ky, A.koff, nprob, d_rmsd0, d_rot0, d_tran0, st, npts);
        fd_launch_metrics(A.ky, A.kx, A.koff, nprob, d_rot0, d_tran0, A.d0, d_met0, st, npts);
    }
    uint64_t *d_mo = (uint64_t *)(R.d_ord + R.o_mo), *d_ro = (uint64_t *)(R.d_ord + R.o_ro);
    if (e == hipSuccess) {
        fd_launch_rs_records_dev(A.matches, nm, A.slot_matches, (uint32_t)I.n_cand, (const uint64_t *)(c->ws[WS_RS_TAB].as<uint32_t>() + L.o_co), A.slot_q, A.qt, (uint32_t)n_queries,
                                 R.d_ord + R.o_scr, d_mo, d_ro, d_rmsd0, d_rot0, d_tran0, d_met0, A.residues, c->ws[WS_RS_REC].p, c->ws[WS_RS_RECRES].as<int32_t>(), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess && nm && !dev_out) e = hipMemcpyAsync(om.p, c->ws[WS_RS_REC].p, nm * sizeof(fd_match_rec), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && tot_res && !dev_out) e = hipMemcpyAsync(orr.p, c->ws[WS_RS_RECRES].p, tot_res * 4, hipMemcpyDeviceToHost, st);
    if (dev_out) { dev_out->got = true; dev_out->recs = c->ws[WS_RS_REC].p; dev_out->residues = c->ws[WS_RS_RECRES].as<int32_t>(); dev_out->n_recs = nm; dev_out->n_res = tot_res; }
    // the two offset arrays lie side by side on the device: one copy into the context's page-locked block, parted on the host
    uint64_t *off_land = d_ro == d_mo + (n_queries + 1) ? (uint64_t *)c->host_pinned(FD_HP_SCAN_B, 2 * (n_queries + 1) * 8) : nullptr;
    if (e == hipSuccess && off_land) e = hipMemcpyAsync(off_land, d_mo, 2 * (n_queries + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !off_land) e = hipMemcpyAsync(omo.p, d_mo, (n_queries + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !off_land) e = hipMemcpyAsync(oro.p, d_ro, (n_queries + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { c->err = std::string("retrieve_batch records: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    if (off_land) { memcpy(omo.p, off_land, (n_queries + 1) * 8); memcpy(oro.p, off_land + (n_queries + 1), (n_queries + 1) * 8); }
    if (I.trace) fprintf(stderr, "[fdgpu_retrieve] device glue: scan %.3f ms (found %llu, cands %llu), group+slots %.3f, superpose + records ordered on the device + copy (%llu records, %llu problems) %.3f\n",
                         t_ms(I.T0, D1), (unsigned long long)R.nf_d, (unsigned long long)R.nc_d, t_ms(D1, D2), (unsigned long long)nm, (unsigned long long)nprob, t_ms(D2, t_now()));
    *out.matches = om.release(); *out.match_off = omo.release(); *out.residues = orr.release(); *out.res_off = oro.release();
    return FDGPU_OK;
}

// -> FDGPU_OK with *done = true and the outputs set; *done = false: the kernel declined (the caller takes the host path).
static int rb_device_glue(const rb_in &I, const rb_out &out, bool *done, fd_rb_dev_out *dev_out) {
    *done = false;
    fdgpu_ctx *c = I.c;
    rs_layout L;
    rs_plan R;
    std::vector<uint32_t> blk_own;
    fd_pair_rec *f_none = nullptr; fd_cand_rec *c_none = nullptr;      // MP_ON_DEVICE: the records stay on the device
    const std::function<void()> pack_tables = [&]() { L = rs_pack_tables(I, blk_own); };
    fd_mp_request rq;
    rq.mode = MP_FOUND | MP_CANDS | MP_ON_DEVICE; rq.while_scanning = &pack_tables;
    int rc = fd_match_pairs_multi(c, I.db, I.resname_std, I.n_queries, I.prep->mqs.data(), I.cand, I.cand_off, I.p, &f_none, &R.nf_d, &c_none, &R.nc_d, rq);
    if (rc) return rc;
    if (!L.blk) pack_tables();
    const rb_time D1 = t_now();
    if ((rc = rs_reserve(I, L, R))) return rc;
    unsigned long long cnt_h[32] = {0};
    if ((rc = rs_launch(I, L, R, cnt_h))) return rc;
    const uint32_t dflags = (uint32_t)cnt_h[4];
    c->last_retrieve_path |= (dflags == 0 ? FDGPU_RPATH_DEVICE_DONE : 0u) | (dflags & 1u ? FDGPU_RPATH_LIMIT : 0u) | (dflags & 2u ? FDGPU_RPATH_CAPACITY : 0u);
    if (dflags) {
        if (I.trace) fprintf(stderr, "[fdgpu_retrieve] device glue declined (flags %u): host path\n", dflags);
        return FDGPU_OK;
    }
    if ((rc = rs_finish(I, L, R, cnt_h, D1, t_now(), out, dev_out))) return rc;
    *done = true;
    return FDGPU_OK;
}

// ------------------------------------------------------------------------------------------ the host path's stages
namespace {
// which way a call goes.  Candidate pairs (the rescue's raw material, retrieve.rs:120-121) number ~ pairs x observed-list entries: a whole-structure
// query makes millions per candidate structure.  Large queries therefore scan twice: found triples only, then — once the
// components and their residue mappings are known — candidate pairs only for partner residues some component mapped
// (the rescue counts nothing else, retrieve.rs:498-511).
struct rb_form {
    bool two_pass = false, dev_glue = false;
    uint32_t path() const { return (two_pass ? FDGPU_RPATH_TWO_PASS : 0u) | (dev_glue ? FDGPU_RPATH_DEVICE_TRIED : 0u); }
};
// a pair scan's output on the host: found / cands are the call's own until the slots are processed (freed here on every return path);
// pk_key / pk_val (packed, device-sorted candidate pairs, fd_match_pairs_multi with MP_CANDS_PACKED) are the context's pinned buffers, not ours to free
struct rb_scan {
    fd_pair_rec *found = nullptr; fd_cand_rec *cands = nullptr; uint64_t nf = 0, nc = 0; uint32_t *pk_key = nullptr, *pk_val = nullptr;
    rb_scan() {}
    rb_scan(const rb_scan &) = delete;
    ~rb_scan() { free(found); free(cands); }
    void drop_cands() { free(cands); cands = nullptr; nc = 0; }
};
// what the helper thread builds while the first scan runs: the hash -> entry tables, the sorted observed-distance lists (two-pass calls)
struct rb_helper_tabs {
    fd_rh_entry_tabs tabs; std::vector<float> sd_dist; std::vector<uint32_t> sd_qi;
    explicit rb_helper_tabs(uint64_t n_queries) : tabs(n_queries) {}
};
struct rb_helper { std::thread t; void join() { if (t.joinable()) t.join(); } ~rb_helper() { join(); } };      // every return path waits for it
// host copies of the coordinates the Kabsch point lists need: every query structure of qb; the candidates' [CA of all | CB of all], slot k at g_dst[k]
struct rb_coords { std::vector<float> qb_ca, qb_cb, t_all; std::vector<uint64_t> g_dst, q_res0; uint64_t g_total = 0; };
// per-slot arrays of the slot passes: slot -> query, the ranges of the scan output at hand, the plan pass's mappings (two-pass calls)
struct rb_slots { std::vector<uint32_t> slot_q, mask_off; std::vector<size_t> f_lo, c_lo; std::vector<fd_rh_slot_plan> plans; };
// rescue votes counted on the device (second scan, fd_match_pairs_multi with MP_VOTES): rows of (largest count, holders, which) per (slot, ordinal,
// query residue) come back instead of the candidate pairs
struct rb_votes { std::vector<uint64_t> row_base; std::vector<fd_vote_row> rows; bool have = false; };
}  // namespace

// stage 2
static rb_form rb_choose_form(const rb_in &I) {
    rb_form F;
    const char *tp_env = getenv("FDGPU_TWO_PASS");     // 1 / 0 force the choice (tests)
    F.two_pass = tp_env ? tp_env[0] == '1' : I.prep->max_aad > 4096;
    const char *hg_env = getenv("FDGPU_HOST_GLUE");      // 1 forces the host path (tests compare the two)
    const uint64_t max_nq = I.prep->max_nq;
    F.dev_glue = !(hg_env && hg_env[0] == '1') && !F.two_pass && !I.partial_fit && max_nq <= FD_WAVE && max_nq > 0 && I.n_cand > 0 && I.n_cand < (1ull << 20);
    return F;
}

// stage 4: the helper thread (large queries: 1 ms for 10^5 hashes, while the scan runs on the GPU), then the first scan — found triples only for a two-pass call
static int rb_first_scan(const rb_in &I, const rb_form &F, rb_helper_tabs &H, rb_helper &helper, fd_mp_tables &mp_tab, rb_scan &S) {
    bool big_tab = false;
    for (uint64_t t = 0; t < I.n_queries; ++t) big_tab = big_tab || I.prep->qhs[t].size() > 4096;
    if (big_tab) {
        const fd_rb_prep *prep = I.prep; const uint64_t n_queries = I.n_queries; const fd_query_map *const *qms = I.qms; const bool two_pass = F.two_pass;
        helper.t = std::thread([prep, n_queries, qms, two_pass, &H]() { fd_rh_build_e_tab(*prep, H.tabs); if (two_pass) fd_rh_build_sorted_lists(n_queries, qms, H.sd_dist, H.sd_qi); });
    }
    fd_mp_request rq;
    rq.mode = F.two_pass ? MP_FOUND : MP_FOUND | MP_CANDS | MP_CANDS_UNORDERED | MP_CANDS_PACKED;
    rq.pk_key = &S.pk_key; rq.pk_val = &S.pk_val; rq.tables = &mp_tab;
    return fd_match_pairs_multi(I.c, I.db, I.resname_std, I.n_queries, I.prep->mqs.data(), I.cand, I.cand_off, I.p, &S.found, &S.nf, &S.cands, &S.nc, rq);
}

// stage 5
static int rb_gather_coords(const rb_in &I, uint64_t nf, rb_coords &X) {
    fdgpu_ctx *c = I.c;
    const fdgpu_batch *qb = I.qb, *db = I.db;
    const uint64_t n_cand = I.n_cand;
    X.qb_ca.assign(std::max<uint64_t>(qb->n_res, 1) * 3, 0.0f); X.qb_cb.assign(X.qb_ca.size(), 0.0f);
    if (qb->n_res) {      // blocking copies on the NULL stream, not on c->stream: they also wait for whatever other streams of the device have queued
        HIPCHK(c, hipMemcpy(X.qb_ca.data(), qb->ca_xyz, qb->n_res * 12, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(X.qb_cb.data(), qb->cb_xyz, qb->n_res * 12, hipMemcpyDeviceToHost));
    }
    X.q_res0.resize(std::max<uint64_t>(I.n_queries, 1));
    for (uint64_t t = 0; t < I.n_queries; ++t) X.q_res0[t] = qb->h_res_off[I.q_struct[t]];
    std::vector<uint64_t> g_src(std::max<uint64_t>(n_cand, 1));
    X.g_dst.assign(n_cand + 1, 0);
    for (uint64_t k = 0; k < n_cand; ++k) {
        g_src[k] = db->h_res_off[I.cand[k]];
        X.g_dst[k + 1] = X.g_dst[k] + (db->h_res_off[I.cand[k] + 1] - db->h_res_off[I.cand[k]]);
    }
    const uint64_t g_total = X.g_total = X.g_dst[n_cand];
    X.t_all.assign(std::max<uint64_t>(6 * g_total, 1), 0.0f);
    if (g_total && nf) {
        HIPCHK(c, c->ws[WS_MISC0].ensure(n_cand * 8));
        HIPCHK(c, c->ws[WS_MISC1].ensure((n_cand + 1) * 8));
        HIPCHK(c, c->ws[WS_MISC2].ensure(6 * g_total * 4));
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC0].p, g_src.data(), n_cand * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC1].p, X.g_dst.data(), (n_cand + 1) * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_gather_xyz, dim3((unsigned)n_cand), dim3(256), 0, c->stream, db->ca_xyz, db->cb_xyz, c->ws[WS_MISC0].as<uint64_t>(),
                           c->ws[WS_MISC1].as<uint64_t>(), g_total, c->ws[WS_MISC2].as<float>());
        HIPCHK(c, hipMemcpyAsync(X.t_all.data(), c->ws[WS_MISC2].p, 6 * g_total * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return FDGPU_OK;
}

// stage 6: the slot ranges of the scan output at hand, then every slot once on the context's pool -> per-slot outputs for the pass's merge
static std::vector<fd_rh_slot_out> rb_run_slots(const rb_in &I, const rb_form &F, const rb_helper_tabs &H, const rb_coords &X, const rb_scan &S, const rb_votes &V,
                                                rb_time T2, bool plan, rb_slots &L) {
    const uint64_t n_cand = I.n_cand;
    fd_rh_slot_ranges(S.found, S.nf, S.cands, S.pk_key, S.nc, n_cand, L.f_lo.data(), L.c_lo.data());
    fd_rh_call C;
    C.qms = I.qms; C.prep = I.prep; C.tabs = &H.tabs; C.cand_off = I.cand_off; C.slot_q = L.slot_q.data();
    C.hash_type = I.p->hash_type; C.node_count = I.node_count; C.trace = I.trace; C.stage_t0 = T2;
    C.found = S.found; C.cands = S.cands; C.pk_key = S.pk_key; C.pk_val = S.pk_val; C.f_lo = L.f_lo.data(); C.c_lo = L.c_lo.data();
    C.t_all = X.t_all.data(); C.g_dst = X.g_dst.data(); C.g_total = X.g_total; C.qb_ca = X.qb_ca.data(); C.qb_cb = X.qb_cb.data(); C.q_res0 = X.q_res0.data();
    if (V.have) { C.vote_rows = V.rows.data(); C.row_base = V.row_base.data(); }
    std::vector<fd_rh_slot_out> outs(n_cand);
    const char *th_env = getenv("FDGPU_HOST_THREADS");
    unsigned n_thr = th_env ? (unsigned)atoi(th_env) : std::min(32u, std::max(1u, std::thread::hardware_concurrency()));
    n_thr = (unsigned)std::min<uint64_t>(std::max(1u, n_thr), std::max<uint64_t>(1, (uint64_t)S.nf / 2048 + 1));   // small jobs stay on the caller's thread
    n_thr = (unsigned)std::min<uint64_t>(n_thr, std::max<uint64_t>(1, n_cand));                                     // a thread per slot at most (spawning one costs ~0.1 ms)
    std::atomic<uint64_t> next(0);
    fd_rh_slot_plan *plans = F.two_pass ? L.plans.data() : nullptr;
    const std::function<void()> worker = [&]() {
        for (uint64_t slot; (slot = next.fetch_add(1)) < n_cand;) fd_rh_slot(C, slot, plan, plans ? plans + slot : nullptr, outs[slot]);
    };
    const rb_time rs_t0 = t_now();
    I.c->host_pool.run(n_thr, worker);      // the context's standing helper threads (a spawn per thread per pass was ~1 ms of the call)
    if (I.trace) fprintf(stderr, "[fdgpu_retrieve] %s pass: %u threads over %llu slots took %.3f ms\n", plan ? "plan" : "full", n_thr, (unsigned long long)n_cand, t_ms(rs_t0, t_now()));
    return outs;
}

// stage 7, votes on the device: the rescue's vote tables fit it (a whole-structure query against its top 20: 20 x 300 x 1,700 counters)
static int rb_scan_device_votes(const rb_in &I, const rb_coords &X, const rb_helper_tabs &H, const fd_rh_marks &M, const std::vector<uint32_t> &mask_off,
                                const std::vector<uint64_t> &vt_off, const std::vector<uint32_t> &vt_qs, uint64_t n_counters, uint64_t n_rows, fd_mp_tables &mp_tab, rb_votes &V) {
    const uint64_t n_cand = I.n_cand;
    std::vector<uint64_t> row_off(n_rows);
    std::vector<uint32_t> row_len(n_rows);
    for (uint64_t k = 0, z = 0; k < n_cand; ++k) {
        const uint32_t Rk = (uint32_t)(X.g_dst[k + 1] - X.g_dst[k]);
        for (uint64_t rr = 0; rr < (uint64_t)M.slot_nrc[k] * vt_qs[k]; ++rr, ++z) { row_off[z] = vt_off[k] + rr * Rk; row_len[z] = Rk; }
    }
    V.rows.resize(std::max<uint64_t>(n_rows, 1));
    fd_vote_plan vp;
    vp.cj_comp = M.cj_comp.data(); vp.n_bits = X.g_total; vp.vt_off = vt_off.data(); vp.vt_qs = vt_qs.data(); vp.n_counters = n_counters;
    vp.row_off = row_off.data(); vp.row_len = row_len.data(); vp.n_rows = n_rows; vp.rows = V.rows.data();
    vp.sd_dist = H.sd_dist.empty() ? nullptr : H.sd_dist.data(); vp.sd_qi = H.sd_qi.empty() ? nullptr : H.sd_qi.data(); vp.n_sd = H.sd_dist.size();
    rb_scan S2;      // nothing of it is kept: the rows are the result
    fd_mp_request rq;
    rq.mode = MP_VOTES; rq.votes = &vp; rq.tables = &mp_tab;
    rq.cj_mask = M.cj_mask.data(); rq.mask_off = mask_off.data(); rq.mask_words = M.cj_mask.size();
    const int rc = fd_match_pairs_multi(I.c, I.db, I.resname_std, I.n_queries, I.prep->mqs.data(), I.cand, I.cand_off, I.p, &S2.found, &S2.nf, &S2.cands, &S2.nc, rq);
    if (rc) return rc;
    V.have = true;
    return FDGPU_OK;
}
// stage 7, the host form: the candidate pairs of the marked partner residues come back (packed when the scan can) for the slots to count
static int rb_scan_host_rescue(const rb_in &I, const fd_rh_marks &M, const std::vector<uint32_t> &mask_off, fd_mp_tables &mp_tab, rb_scan &S) {
    rb_scan S2;
    fd_mp_request rq;
    rq.mode = MP_CANDS | MP_CANDS_UNORDERED | MP_CANDS_PACKED; rq.pk_key = &S.pk_key; rq.pk_val = &S.pk_val; rq.tables = &mp_tab;
    rq.cj_mask = M.cj_mask.data(); rq.mask_off = mask_off.data(); rq.mask_words = M.cj_mask.size();
    const int rc = fd_match_pairs_multi(I.c, I.db, I.resname_std, I.n_queries, I.prep->mqs.data(), I.cand, I.cand_off, I.p, &S2.found, &S2.nf, &S2.cands, &S2.nc, rq);
    std::swap(S.cands, S2.cands); S.nc = S2.nc;      // (S.cands was dropped before the scan: S2 leaves with nothing but its found triples)
    return rc;
}
// stage 7: the second scan of a two-pass call, in the form the plan pass's marks allow
static int rb_second_scan(const rb_in &I, const rb_coords &X, const rb_helper_tabs &H, const fd_rh_marks &M, const rb_slots &L, rb_time T2, fd_mp_tables &mp_tab, rb_scan &S, rb_votes &V) {
    const uint64_t n_cand = I.n_cand;
    uint64_t n_counters = 0, n_rows = 0;
    std::vector<uint64_t> vt_off(n_cand + 1, 0);
    std::vector<uint32_t> vt_qs(n_cand + 1, 0);
    for (uint64_t k = 0; k < n_cand; ++k) {
        vt_off[k] = n_counters; V.row_base[k] = n_rows; vt_qs[k] = I.prep->q_sizes[L.slot_q[k]];
        n_counters += (uint64_t)M.slot_nrc[k] * vt_qs[k] * (X.g_dst[k + 1] - X.g_dst[k]);
        n_rows += (uint64_t)M.slot_nrc[k] * vt_qs[k];
    }
    const char *dv_env = getenv("FDGPU_DEVICE_VOTES");      // 0: the rescue counts on the host from the copied candidate pairs (tests)
    const bool dev_votes = M.any_rescue && !M.vote_conflict && !(dv_env && dv_env[0] == '0') && n_counters <= (1ull << 28) && n_rows <= (1ull << 24) &&
                           X.g_total < (1ull << 32);
    int rc = FDGPU_OK;
    if (dev_votes) {
        if ((rc = rb_scan_device_votes(I, X, H, M, L.mask_off, vt_off, vt_qs, n_counters, n_rows, mp_tab, V))) return rc;
        if (I.trace) fprintf(stderr, "[fdgpu_retrieve] second scan (device votes) done at %.3f ms (%llu rows)\n", t_ms(T2, t_now()), (unsigned long long)n_rows);
    } else if (M.any_rescue) {
        if ((rc = rb_scan_host_rescue(I, M, L.mask_off, mp_tab, S))) return rc;
        if (I.trace) fprintf(stderr, "[fdgpu_retrieve] second scan done at %.3f ms (cands %llu)\n", t_ms(T2, t_now()), (unsigned long long)S.nc);
    }
    return FDGPU_OK;
}
// unpacked fallback (>= 2^16 candidate slots): atomic-append order -> grouped by candidate slot (counting sort)
static int rb_regroup_unpacked(uint64_t n_cand, rb_scan &S) {
    std::vector<uint64_t> so(n_cand + 2, 0);
    for (uint64_t e = 0; e < S.nc; ++e) ++so[S.cands[e].cand + 1];
    for (uint64_t k = 0; k < n_cand; ++k) so[k + 1] += so[k];
    fd_cand_rec *g2 = (fd_cand_rec *)malloc(S.nc * sizeof(fd_cand_rec));
    if (!g2) return FDGPU_ENOMEM;
    for (uint64_t e = 0; e < S.nc; ++e) g2[so[S.cands[e].cand]++] = S.cands[e];
    free(S.cands); S.cands = g2;
    return FDGPU_OK;
}

// stage 9: one Kabsch batch over every problem of the call, the optional LMS override, the metrics, the records filled
static int rb_superpose(const rb_in &I, fd_rh_merged &R, uint64_t nf, uint64_t nc, rb_time T1, rb_time T2) {
    fdgpu_ctx *c = I.c;
    std::vector<fd_match_rec> &recs = R.recs;
    const std::vector<float> &kx = R.kx, &ky = R.ky;
    const std::vector<uint64_t> &koff = R.koff;
    const uint64_t nprob = R.pend.size();
    std::vector<float> rmsd(std::max<uint64_t>(nprob, 1)), rot(std::max<uint64_t>(nprob, 1) * 9), tran(std::max<uint64_t>(nprob, 1) * 3);
    const rb_time T3 = t_now();
    int rc = 0;
    if (nprob && (rc = fdgpu_kabsch_batch(c, kx.data(), ky.data(), koff.data(), nprob, rmsd.data(), rot.data(), tran.data()))) return rc;
    if (I.partial_fit && nprob) {   // --partial-fit: mappings of more than 3 residues take the LMS fit instead (retrieve.rs:733-746)
        std::vector<uint64_t> which, loff(1, 0);
        std::vector<float> lx, ly;
        for (uint64_t k = 0; k < nprob; ++k) {
            const uint64_t a = koff[k], b = koff[k + 1];
            if (b - a <= 6) continue;                       // [CA, CB] per residue: index1.len() <= 3 keeps Kabsch
            which.push_back(k);
            lx.insert(lx.end(), kx.begin() + 3 * a, kx.begin() + 3 * b);
            ly.insert(ly.end(), ky.begin() + 3 * a, ky.begin() + 3 * b);
            loff.push_back(loff.back() + (b - a));
        }
        if (!which.empty()) {
            std::vector<float> lr(which.size()), lrot(which.size() * 9), ltr(which.size() * 3);
            if ((rc = fdgpu_lms_qcp_batch(c, lx.data(), ly.data(), loff.data(), which.size(), lr.data(), lrot.data(), ltr.data(), nullptr, nullptr)))
                return rc;
            for (size_t z = 0; z < which.size(); ++z) {
                rmsd[which[z]] = lr[z];
                memcpy(&rot[9 * which[z]], &lrot[9 * z], 36);
                memcpy(&tran[3 * which[z]], &ltr[3 * z], 12);
            }
        }
    }
    if (I.trace) fprintf(stderr, "[fdgpu_retrieve] match_pairs %.3f ms (found %llu, cands %llu), gather %.3f, graph/vote %.3f, kabsch(%llu) %.3f\n", t_ms(I.T0, T1),
                         (unsigned long long)nf, (unsigned long long)nc, t_ms(T1, T2), t_ms(T2, T3), (unsigned long long)nprob, t_ms(T3, t_now()));
    // similarity metrics of every superposition on the device (k_metrics), after a possible --partial-fit override of rot / tran
    std::vector<float> mets(std::max<uint64_t>(nprob, 1) * 5);
    if (nprob && (rc = fdgpu_metrics_batch(c, ky.data(), kx.data(), koff.data(), nprob, rot.data(), tran.data(), mets.data()))) return rc;
    for (uint64_t k = 0; k < nprob; ++k) {
        fd_match_rec &r = recs[R.pend[k].rec];
        const bool is_out = R.pend[k].which == 1 || r.same;   // the superposition the match reports
        if (R.pend[k].which == 0) {
            r.rmsd_from_hash = rmsd[k]; memcpy(r.rot_from_hash, &rot[9 * k], 36); memcpy(r.tran_from_hash, &tran[3 * k], 12);
            memcpy(r.metrics_from_hash, &mets[5 * k], 20);
        }
        if (is_out) {
            r.rmsd = rmsd[k]; memcpy(r.rot, &rot[9 * k], 36); memcpy(r.tran, &tran[3 * k], 12);
            memcpy(r.metrics, &mets[5 * k], 20);
        }
    }
    return FDGPU_OK;
}

// stage 10
static int rb_hand_out(uint64_t n_queries, const fd_rh_merged &R, const rb_out &out) {
    rb_owned<fd_match_rec> om((fd_match_rec *)malloc(std::max<size_t>(R.recs.size(), 1) * sizeof(fd_match_rec)));
    rb_owned<int32_t> orr((int32_t *)malloc(std::max<size_t>(R.res.size(), 1) * sizeof(int32_t)));
    rb_owned<uint64_t> omo((uint64_t *)malloc((n_queries + 1) * 8)), oro((uint64_t *)malloc((n_queries + 1) * 8));
    if (!om.p || !orr.p || !omo.p || !oro.p) return FDGPU_ENOMEM;
    if (!R.recs.empty()) memcpy(om.p, R.recs.data(), R.recs.size() * sizeof(fd_match_rec));
    if (!R.res.empty()) memcpy(orr.p, R.res.data(), R.res.size() * sizeof(int32_t));
    memcpy(omo.p, R.m_off.data(), (n_queries + 1) * 8);
    memcpy(oro.p, R.r_off.data(), (n_queries + 1) * 8);
    *out.matches = om.release(); *out.match_off = omo.release(); *out.residues = orr.release(); *out.res_off = oro.release();
    return FDGPU_OK;
}

// retrieval_wrapper for MANY queries: one pair scan, one coordinate gather and one Kabsch launch in total.  Query t = structure
// q_struct[t] of qb with the query map qms[t]; its candidates are cand[cand_off[t] .. cand_off[t+1]).  Matches of query t:
// (*matches)[(*match_off)[t] .. (*match_off)[t+1]) (cand = slot inside the query's own candidate list), residues
// (*residues)[(*res_off)[t] ...], 2 * n_indices(t) per match.
// prep: the maps' tables when the caller has built them already (fd_rb_prepare with the same maps and ca_distance_cutoff), else null
static int fd_retrieve_batch_impl(fdgpu_ctx *c, const fdgpu_batch *db, const uint8_t *resname_std, uint64_t n_queries, const uint32_t *cand,
                                  const uint64_t *cand_off, const fd_query_map *const *qms, const fdgpu_batch *qb, const uint32_t *q_struct,
                                  const fd_hash_params *p, float ca_distance_cutoff, uint32_t node_count, uint32_t partial_fit, fd_match_rec **matches,
                                  uint64_t **match_off, int32_t **residues, uint64_t **res_off, const fd_rb_prep *prep, fd_rb_dev_out *dev_out = nullptr) { FD_LOCK(c);
    // 1. validate
    if (c) c->last_retrieve_path = 0;      // also for a call rejected below: the flags describe the LAST call
    if (!c || !db || !qb || !p || !matches || !match_off || !residues || !res_off || !cand_off || (n_queries && (!qms || !q_struct))) return FDGPU_EINVAL;
    *matches = nullptr; *match_off = nullptr; *residues = nullptr; *res_off = nullptr;
    for (uint64_t t = 0; t < n_queries; ++t) if (!qms[t] || q_struct[t] >= qb->n_struct) return FDGPU_EINVAL;
    fd_rb_prep prep_own;
    rb_in I = {c, db, resname_std, n_queries, cand, cand_off, qms, qb, q_struct, p, node_count, partial_fit, cand_off[n_queries], prep, getenv("FDGPU_TRACE") != nullptr, t_now()};
    if (!prep) { fd_rb_prepare(n_queries, qms, ca_distance_cutoff, prep_own); I.prep = &prep_own; }
    const rb_out out = {matches, match_off, residues, res_off};
    const uint64_t n_cand = I.n_cand;
    // 2. the form, 3. the device glue
    const rb_form F = rb_choose_form(I);
    c->last_retrieve_path = F.path();
    int rc = 0;
    if (F.dev_glue) {
        bool done = false;
        rc = rb_device_glue(I, out, &done, dev_out);
        if (rc || done) return rc;
    }
    if (I.trace) fprintf(stderr, "[fdgpu_retrieve] query tables %.3f ms\n", t_ms(I.T0, t_now()));
    // 4. helper thread + first scan, 5. coordinates
    rb_helper_tabs H(n_queries);
    rb_helper helper;         // (behind H: joined before the tables it fills go away)
    fd_mp_tables mp_tab;      // work items + query tables: built by the first scan, reused by the second
    rb_scan S;
    if ((rc = rb_first_scan(I, F, H, helper, mp_tab, S))) return rc;
    const rb_time T1 = t_now();
    rb_coords X;
    if ((rc = rb_gather_coords(I, S.nf, X))) return rc;
    const rb_time T2 = t_now();
    // 6. - 8. per candidate: graph -> components -> vote -> rescue; Kabsch problems collected for one GPU batch
    rb_slots L;
    L.slot_q.assign(std::max<uint64_t>(n_cand, 1), 0);
    for (uint64_t t = 0; t < n_queries; ++t) for (uint64_t k = cand_off[t]; k < cand_off[t + 1]; ++k) L.slot_q[k] = (uint32_t)t;
    L.mask_off.assign(n_cand + 1, 0);
    for (uint64_t k = 0; k < n_cand; ++k) L.mask_off[k] = (uint32_t)X.g_dst[k];
    L.f_lo.assign(n_cand + 1, 0); L.c_lo.assign(n_cand + 1, 0);
    L.plans.resize(F.two_pass ? n_cand : 0);
    rb_votes V;
    V.row_base.assign(n_cand + 1, 0);
    helper.join();
    if (F.two_pass) {
        fd_rh_marks M;
        M.cj_mask.assign((X.g_total + 31) / 32 + 1, 0); M.cj_comp.assign(X.g_total + 1, 0); M.slot_nrc.assign(n_cand + 1, 0);
        fd_rh_merge_plan(rb_run_slots(I, F, H, X, S, V, T2, true, L), L.mask_off.data(), M);
        if (I.trace) fprintf(stderr, "[fdgpu_retrieve] plan pass %.3f ms\n", t_ms(T2, t_now()));
        S.drop_cands();
        if ((rc = rb_second_scan(I, X, H, M, L, T2, mp_tab, S, V))) return rc;
    }
    if (S.nc && !S.pk_key && (rc = rb_regroup_unpacked(n_cand, S))) return rc;
    fd_rh_merged R;
    fd_rh_merge_full(rb_run_slots(I, F, H, X, S, V, T2, false, L), n_queries, cand_off, R);
    if (I.trace) fprintf(stderr, "[fdgpu_retrieve] slots done at %.3f ms\n", t_ms(T2, t_now()));
    const uint64_t nf = S.nf, nc = S.nc;
    free(S.found); S.found = nullptr; S.drop_cands();      // tens of MB for a whole-structure query: not held through the superposition
    // 9. superpose, 10. hand out
    if ((rc = rb_superpose(I, R, nf, nc, T1, T2))) return rc;
    return rb_hand_out(n_queries, R, out);
}
int fd_retrieve_batch_dev(fdgpu_ctx *c, const fdgpu_batch *db, const uint8_t *resname_std, uint64_t n_queries, const uint32_t *cand, const uint64_t *cand_off,
                          const fd_query_map *const *qms, const fdgpu_batch *qb, const uint32_t *q_struct, const fd_hash_params *p, float ca_distance_cutoff,
                          uint32_t node_count, uint32_t partial_fit, fd_match_rec **matches, uint64_t **match_off, int32_t **residues, uint64_t **res_off, fd_rb_dev_out *dev) { FD_LOCK(c);
    if (dev) *dev = fd_rb_dev_out();
    return fd_retrieve_batch_impl(c, db, resname_std, n_queries, cand, cand_off, qms, qb, q_struct, p, ca_distance_cutoff, node_count, partial_fit, matches, match_off,
                                  residues, res_off, nullptr, dev);
}
extern "C" int fdgpu_retrieve_batch(fdgpu_ctx *c, const fdgpu_batch *db, const uint8_t *resname_std, uint64_t n_queries, const uint32_t *cand,
                                    const uint64_t *cand_off, const fd_query_map *const *qms, const fdgpu_batch *qb, const uint32_t *q_struct,
                                    const fd_hash_params *p, float ca_distance_cutoff, uint32_t node_count, uint32_t partial_fit, fd_match_rec **matches,
                                    uint64_t **match_off, int32_t **residues, uint64_t **res_off) { FD_LOCK(c);
    return fd_retrieve_batch_impl(c, db, resname_std, n_queries, cand, cand_off, qms, qb, q_struct, p, ca_distance_cutoff, node_count, partial_fit, matches, match_off,
                                  residues, res_off, nullptr);
}
extern "C" int fdgpu_debug_last_retrieve_path(fdgpu_ctx *c, uint32_t *flags) { FD_LOCK(c);
    if (!c || !flags) return FDGPU_EINVAL;
    *flags = c->last_retrieve_path;
    return FDGPU_OK;
}

// The body of query_pdb.rs:376-452 for a batch of queries in ONE call: query maps -> scoring + ranked top_n -> retrieval of every query's first
// match_top candidates.  Same results as fdgpu_make_query_map_batch + fdgpu_count_query_maps_top + fdgpu_retrieve_batch called one after the other
// (tests compare them bit for bit); what the call adds is overlap the three blocking calls cannot have: the retrieval's query tables are built
// while the scoring kernels run, only the candidates' ids (match_top per query) are waited for before the pair scan starts, and the ranked records
// (n_queries x top_n x 20 bytes) cross the bus on a second stream while the retrieval's kernels run.
extern "C" int fdgpu_query_batch(fdgpu_ctx *c, const fdgpu_index *ix, const fdgpu_batch *db, const uint8_t *resname_std, const fdgpu_batch *qb, uint64_t n_queries,
                                 const uint32_t *q_struct, const uint64_t *q_off, const uint32_t *q_index, const uint8_t *const *subs, const uint32_t *n_subs,
                                 const float *dist_thr, uint64_t n_dist, const float *angle_thr_deg, uint64_t n_angle, const fd_hash_params *p, float total_structures,
                                 const float *penalty, uint32_t top_n, uint32_t match_top, float ca_distance_cutoff, uint32_t node_count, fd_query_map **maps,
                                 fd_count_rec **recs, uint64_t **rec_off, fd_match_rec **matches, uint64_t **match_off, int32_t **residues, uint64_t **res_off) { FD_LOCK(c);
    if (!c || !ix || !db || !qb || !p || !maps || !recs || !rec_off || !matches || !match_off || !residues || !res_off || !q_off || (n_queries && !q_struct)) return FDGPU_EINVAL;
    *recs = nullptr; *rec_off = nullptr; *matches = nullptr; *match_off = nullptr; *residues = nullptr; *res_off = nullptr;
    int rc = fdgpu_make_query_map_batch(c, qb, n_queries, q_struct, q_off, q_index, subs, n_subs, dist_thr, n_dist, angle_thr_deg, n_angle, p, ix, total_structures, maps);
    if (rc) return rc;
    auto drop_maps = [&]() { for (uint64_t t = 0; t < n_queries; ++t) { fdgpu_query_map_free(maps[t]); maps[t] = nullptr; } };
    fd_rb_prep prep;
    bool prep_done = false;
    const std::function<void()> build_prep = [&]() { fd_rb_prepare(n_queries, maps, ca_distance_cutoff, prep); prep_done = true; };
    fd_cq_dev_out D;
    D.while_running = &build_prep;
    D.head_n = std::min(match_top, top_n);
    fd_count_rec *rr = nullptr;
    uint64_t *roff = nullptr;
    rc = fd_count_query_maps_top_impl(c, ix, n_queries, maps, penalty, total_structures, top_n, &rr, &roff, &D);
    if (!rc && D.got && D.overflow) {      // more ties at a cut-off than the device selection holds: the compacting path, host records
        fdgpu_free(rr); free(roff); rr = nullptr; roff = nullptr;
        rc = fd_count_query_maps_top_impl(c, ix, n_queries, maps, penalty, total_structures, top_n, &rr, &roff, nullptr, /*allow_dense=*/false);
        D.got = false;
    }
    if (rc) { drop_maps(); return rc; }
    if (!prep_done) build_prep();
    std::vector<uint32_t> cand;
    std::vector<uint64_t> cand_off(n_queries + 1, 0);
    const uint64_t first = ix->first_id;
    bool side_copy = false;
    if (D.got) {
        // the candidates: the first match_top records of every query's ranking (a strided copy of 20 x match_top bytes per query)
        hipStream_t st = c->stream;
        const uint32_t mt = std::min(match_top, top_n);
        std::vector<fd_count_rec> head_v;
        const size_t head_bytes = (size_t)n_queries * std::max<uint32_t>(mt, 1) * sizeof(fd_count_rec);
        const fd_count_rec *head = D.head;       // came with the selection's state (one wait)
        hipError_t e = hipSuccess;
        if (!head) {
            fd_count_rec *h2 = (fd_count_rec *)c->host_pinned(FD_HP_UP, head_bytes);
            if (!h2) { head_v.resize((size_t)n_queries * std::max<uint32_t>(mt, 1)); h2 = head_v.data(); }
            if (mt && n_queries)
                e = hipMemcpy2DAsync(h2, (size_t)mt * sizeof(fd_count_rec), D.recs, (size_t)top_n * sizeof(fd_count_rec), (size_t)mt * sizeof(fd_count_rec), n_queries,
                                     hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            head = h2;
        }
        // the full ranking: straight into the caller's (page-locked, pooled) array on the second stream, closed up after the retrieval
        rr = (fd_count_rec *)fd_out_alloc(std::max<uint64_t>((uint64_t)n_queries * top_n, 1) * sizeof(fd_count_rec), true);
        roff = (uint64_t *)calloc(n_queries + 1, 8);
        if (e == hipSuccess && (!rr || !roff)) { fdgpu_free(rr); free(roff); drop_maps(); return FDGPU_ENOMEM; }
        if (e == hipSuccess && !c->side_stream) e = hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking);
        if (e == hipSuccess && n_queries && top_n) {
            e = hipMemcpyAsync(rr, D.recs, (size_t)n_queries * top_n * sizeof(fd_count_rec), hipMemcpyDeviceToHost, c->side_stream);
            side_copy = e == hipSuccess;
        }
        if (e != hipSuccess) {
            if (side_copy) (void)hipStreamSynchronize(c->side_stream);
            fdgpu_free(rr); free(roff); drop_maps();
            c->err = std::string("query_batch: ") + hipGetErrorString(e);
            return FDGPU_EHIP;
        }
        for (uint64_t t = 0; t < n_queries; ++t) {
            const uint32_t m = std::min<uint32_t>(std::min<uint32_t>(D.counts[t], top_n), mt);
            for (uint32_t k = 0; k < m; ++k) cand.push_back((uint32_t)(head[(size_t)t * mt + k].nid - first));
            cand_off[t + 1] = cand.size();
        }
    } else {
        for (uint64_t t = 0; t < n_queries; ++t) {
            const uint64_t m = std::min<uint64_t>(roff[t + 1] - roff[t], match_top);
            for (uint64_t k = 0; k < m; ++k) cand.push_back((uint32_t)(rr[roff[t] + k].nid - first));
            cand_off[t + 1] = cand.size();
        }
    }
    rc = fd_retrieve_batch_impl(c, db, resname_std, n_queries, cand.data(), cand_off.data(), maps, qb, q_struct, p, ca_distance_cutoff, node_count, 0, matches, match_off,
                                residues, res_off, &prep);
    if (side_copy) {
        // the side-stream copy read WS_TILE_HO while the retrieval ran: correct only as long as no retrieval stage grows (= frees) or writes that buffer
        if (c->ws[WS_TILE_HO].p != D.recs && !rc) { c->err = "query_batch: a retrieval stage re-allocated the ranking's buffer under its copy"; rc = FDGPU_EHIP; }
        const hipError_t e = hipStreamSynchronize(c->side_stream);
        if (e != hipSuccess && !rc) { c->err = std::string("query_batch records: ") + hipGetErrorString(e); rc = FDGPU_EHIP; }
    }
    if (!rc && D.got) {       // close the fixed-stride ranking up in place (forward moves: the write position never passes the read position)
        uint64_t w = 0;
        for (uint64_t t = 0; t < n_queries; ++t) {
            const uint64_t m = std::min<uint32_t>(D.counts[t], top_n);
            roff[t] = w;
            if (m && w != t * top_n) memmove(rr + w, rr + (size_t)t * top_n, (size_t)m * sizeof(fd_count_rec));
            w += m;
        }
        roff[n_queries] = w;
    }
    if (rc) {
        fdgpu_free(rr); free(roff); drop_maps();
        fdgpu_free(*matches); fdgpu_free(*residues); free(*match_off); free(*res_off);
        *matches = nullptr; *match_off = nullptr; *residues = nullptr; *res_off = nullptr;
        return rc;
    }
    *recs = rr; *rec_off = roff;
    return FDGPU_OK;
}

// one query = structure 0 of qb
extern "C" int fdgpu_retrieve(fdgpu_ctx *c, const fdgpu_batch *db, const uint8_t *resname_std, const uint32_t *cand, uint64_t n_cand,
                              const fd_query_map *qm, const fdgpu_batch *qb, const fd_hash_params *p, float ca_distance_cutoff,
                              uint32_t node_count, uint32_t partial_fit, fd_match_rec **matches, uint64_t *n_matches, int32_t **residues) { FD_LOCK(c);
    if (!c || !db || !qm || !qb || !p || !matches || !n_matches || !residues) return FDGPU_EINVAL;
    *matches = nullptr; *n_matches = 0; *residues = nullptr;
    const uint64_t off[2] = {0, n_cand};
    const uint32_t s0 = 0;
    uint64_t *mo = nullptr, *ro = nullptr;
    int rc = fdgpu_retrieve_batch(c, db, resname_std, 1, cand, off, &qm, qb, &s0, p, ca_distance_cutoff, node_count, partial_fit, matches, &mo, residues, &ro);
    if (rc) return rc;
    *n_matches = mo[1];
    free(mo); free(ro);
    return FDGPU_OK;
}


// ------------------------------------------------------------------------------------------ sub-index merge
// Index build shards by structure (one sub-index per GPU / per batch, contiguous ascending id ranges).  The
// reference's single on-disk index is the per-hash concatenation of the shards' posting lists in shard order;
// only the first varint of every continuation (an absolute id in its own sub-index) must be re-encoded as the
// delta from the last id of the list so far (src/index/indextable.rs:171-202 semantics).  Host-side, streaming.
static inline uint64_t fd_decode_last(const uint8_t *b, uint64_t n, uint64_t *first_len, uint64_t *first_val) {
    uint64_t acc = 0, prev = 0, cur = 0;
    unsigned shift = 0;
    bool first = true;
    for (uint64_t k = 0; k < n; ++k) {
        acc |= (uint64_t)(b[k] & 0x7f) << shift;
        if (b[k] & 0x80) { shift += 7; continue; }
        if (first) { cur = acc; *first_len = k + 1; *first_val = acc; first = false; }
        else cur = prev + acc;
        prev = cur; acc = 0; shift = 0;
    }
    return cur;
}

extern "C" int fdgpu_merge_subindices(uint64_t n_parts, const uint8_t *const *values, const uint32_t *const *hashes,
                                      const uint64_t *const *offsets, const uint64_t *n_hashes, uint8_t **out_value, uint64_t *out_value_len,
                                      uint32_t **out_hashes, uint64_t **out_offsets, uint64_t *out_n_hashes) {
    if (!values || !hashes || !offsets || !n_hashes || !out_value || !out_value_len || !out_hashes || !out_offsets || !out_n_hashes) return FDGPU_EINVAL;
    uint64_t tot_h = 0, tot_v = 0;
    for (uint64_t p = 0; p < n_parts; ++p) { tot_h += n_hashes[p]; tot_v += offsets[p][n_hashes[p]]; }
    uint8_t *V = (uint8_t *)malloc(std::max<uint64_t>(tot_v + 8, 8));          // re-based first deltas are never longer than the absolute ids
    uint32_t *H = (uint32_t *)malloc(std::max<uint64_t>(tot_h, 1) * 4);
    uint64_t *O = (uint64_t *)malloc((tot_h + 1) * 8);
    if (!V || !H || !O) { free(V); free(H); free(O); return FDGPU_ENOMEM; }
    std::vector<uint64_t> pos(n_parts, 0);
    uint64_t nh = 0, nv = 0;
    O[0] = 0;
    for (;;) {
        bool any = false;
        uint32_t hmin = 0;
        for (uint64_t p = 0; p < n_parts; ++p)
            if (pos[p] < n_hashes[p] && (!any || hashes[p][pos[p]] < hmin)) { hmin = hashes[p][pos[p]]; any = true; }
        if (!any) break;
        bool have_last = false;
        uint64_t last = 0;
        for (uint64_t p = 0; p < n_parts; ++p) {   // shard order = ascending id ranges
            if (pos[p] >= n_hashes[p] || hashes[p][pos[p]] != hmin) continue;
            const uint8_t *b = values[p] + offsets[p][pos[p]];
            uint64_t len = offsets[p][pos[p] + 1] - offsets[p][pos[p]];
            uint64_t flen = 0, fval = 0;
            uint64_t lst = fd_decode_last(b, len, &flen, &fval);
            if (!have_last) { memcpy(V + nv, b, len); nv += len; }
            else {
                if (fval <= last) { free(V); free(H); free(O); return FDGPU_EINVAL; }   // id ranges must ascend across parts
                nv += fd_put_varint(fval - last, V + nv);
                memcpy(V + nv, b + flen, len - flen); nv += len - flen;
            }
            last = lst; have_last = true;
            ++pos[p];
        }
        H[nh] = hmin; O[++nh] = nv;
    }
    *out_value = V; *out_value_len = nv; *out_hashes = H; *out_offsets = O; *out_n_hashes = nh;
    return FDGPU_OK;
}


// ---- analyze: hypergeometric enrichment of encodings (src/controller/summary.rs:543-628) --------------------------------------------
// p[k] = P(X >= x) for X ~ Hypergeometric(N = total_bg + total_query, K = bg[k] + query[k], n = total_query), x = query[k]: the sum of
// the log-space pmf from x to min(n, K) with the reference's log-factorial (exact sum of ln below 20, Stirling's formula above,
// summary.rs:616-628), clamped to 1.  The terms fall monotonically behind the mode, so the walk stops once a term no longer changes
// the f64 sum — the value is the one the full loop gives.  Host threads over the encodings.
namespace {
inline double fd_log_factorial(uint64_t n) {
    if (n <= 1) return 0.0;
    if (n < 20) { double s = 0.0; for (uint64_t i = 2; i <= n; ++i) s += log((double)i); return s; }
    const double x = (double)n;
    return x * log(x) - x + 0.5 * log(2.0 * 3.14159265358979323846 * x);
}
inline double fd_log_binomial(uint64_t n, uint64_t k) {
    if (k > n) return -INFINITY;
    if (k == 0 || k == n) return 0.0;
    return fd_log_factorial(n) - fd_log_factorial(k) - fd_log_factorial(n - k);
}
}
extern "C" int fdgpu_hypergeom_enrichment(const uint64_t *query_count, const uint64_t *bg_count, uint64_t n_enc, uint64_t total_query, uint64_t total_bg,
                                          uint32_t n_threads, double *p_value) {
    if (n_enc && (!query_count || !bg_count || !p_value)) return FDGPU_EINVAL;
    const uint64_t n = total_query, N = total_bg + total_query;
    const double log_den = fd_log_binomial(N, n);
    auto work = [&](uint64_t a, uint64_t b) {
        for (uint64_t e = a; e < b; ++e) {
            const uint64_t x = query_count[e], K = bg_count[e] + query_count[e], max_x = n < K ? n : K;
            const double mode = (double)(n + 1) * (double)(K + 1) / (double)(N + 2);
            double p = 0.0;
            for (uint64_t i = x; i <= max_x; ++i) {
                const double t = exp(fd_log_binomial(K, i) + fd_log_binomial(N - K, n - i) - log_den);
                const double q = p + t;
                if (q == p && (double)i > mode) break;
                p = q;
            }
            p_value[e] = p < 1.0 ? p : 1.0;
        }
    };
    const uint32_t T = std::max<uint32_t>(1, std::min<uint32_t>(n_threads ? n_threads : 1, 256));
    if (T == 1 || n_enc < 64) { work(0, n_enc); return FDGPU_OK; }
    std::vector<std::thread> th;
    const uint64_t per = (n_enc + T - 1) / T;
    for (uint32_t t = 0; t < T; ++t) { const uint64_t a = (uint64_t)t * per, b = std::min<uint64_t>(n_enc, a + per); if (a < b) th.emplace_back(work, a, b); }
    for (auto &x : th) x.join();
    return FDGPU_OK;
}
