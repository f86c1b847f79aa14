// k_overlap.hip — exact row overlaps: device-resident row sets (fdgpu_index_rowset, _info, _lengths, _export, _destroy) and the pair intersect
// (fdgpu_rowset_intersect); the definitions are include/fdgpu.h, the host form fd_overlap_host.cpp, the account DESIGN.md §4j.
//
// A row set holds the rows of chosen structures of one index.  Its storage is segmented: one block per window of the walk, the window's taken
// rows back to back in it, plus two device tables over all rows: row_ptr[k] (where row k starts, a device address) and row_len[k].  Nothing
// is sized before a window has run, and a consumer needs no segment arithmetic.  Per window:
//   rows          fd_rows_device (k_rows.hip) as it is: the window's rows in the context's workspaces
//   k_ro_lens     thread per wanted row: len[j] = row_off[slot[j] + 1] - row_off[slot[j]]
//   scan          the shared exclusive scan: dst[j] = where wanted row j starts in the block, dst[m] = their sum.  dst comes to the host, which
//                 applies the budget rule (a prefix of the wanted rows is taken) and takes the block from the indices' allocator
//   k_ro_gather   wavefront per taken row: the lanes stride the row (coalesced 256-byte reads and writes), lane 0 writes the row's two table
//                 entries.  No atomic: every destination comes from the scan
// The full rows of a window stay in the workspaces and are overwritten by the next window.
//
// The intersect: two ascending lists of distinct u32, 0 to more than 10^5 elements each.
//   k_ov_plan     thread per pair: key = the power-of-two class of |R_a| + |R_b|, smaller key = longer
//   sort          one stable radix pass (6 key bits) in the sort workspaces: the pairs longest class first, input order inside a class.  A long
//                 pair is one wavefront's serial walk; started first, it overlaps the many short ones instead of trailing them
//   k_ov_pairs    wavefront per pair, four per workgroup.  Both rows are consumed in tiles of 64 read coalesced (lane i reads element i of the
//                 tile), the tile after the current one of each row already on its way.  The B tile lies in the wavefront's own 64 words of LDS;
//                 every lane looks its A element up there by bisection over the tile's LENGTH — a partial tile is masked by its length, never
//                 padded with a value, since every u32 is a legal hash — and a ballot's popcount accumulates.  The tile with the smaller last
//                 element advances, both on a tie.  One store per pair, to the pair's input slot.
// Why this is exact: rows hold distinct ascending values, so a common value x lies in exactly one A tile i and one B tile j, and the walk visits
// (i, j): it cannot leave row i at an earlier B tile j' (that needs last_a(i) <= last_b(j') < x) nor pass column j before reaching row i (that
// needs last_b(j) <= last_a(i') < x).  Every (A tile, B tile) combination is visited at most once, so x is counted once.  The count is a pure
// function of the two lists: no global atomic, no dependence on the launch geometry or on the order of the pairs.
// Workspace: 12 bytes per row of a set (tables) + 4 per wanted row and window (slot, len) + 8 (dst); 8 + 16 + 4 bytes per pair (slots, sort, result).
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include "fdgpu_internal.h"
#include "fd_api_common.h"

#define OV_WINDOW_DEFAULT 16384u
#define OV_TILE 64u
#define OV_KEY_BITS 6

extern "C" void fdgpu_rowset_destroy(fdgpu_rowset *rs) {
    if (!rs) return;
    FD_LOCK(rs->ctx);     // the blocks go back to the context's pool
    for (auto &b : rs->blocks) rs->ctx->pool_free(b.p, b.cap);
    rs->ctx->pool_free(rs->row_ptr, rs->cap_ptr);
    rs->ctx->pool_free(rs->row_len, rs->cap_len);
    delete rs;
}

extern "C" int fdgpu_rowset_info(const fdgpu_rowset *rs, uint64_t *n_rows, uint64_t *n_hashes) {
    if (!rs) return FDGPU_EINVAL;
    if (n_rows) *n_rows = rs->n_rows;
    if (n_hashes) *n_hashes = rs->n_hashes;
    return FDGPU_OK;
}

extern "C" int fdgpu_rowset_lengths(const fdgpu_rowset *rs, uint32_t **lengths) {
    if (!rs || !lengths) return FDGPU_EINVAL;
    *lengths = (uint32_t *)fd_out_alloc(std::max<uint64_t>(rs->n_rows, 1) * 4);
    if (!*lengths) return FDGPU_ENOMEM;
    (*lengths)[0] = 0;
    if (rs->n_rows) memcpy(*lengths, rs->h_len.data(), rs->n_rows * 4);
    return FDGPU_OK;
}

// ---- lens: thread per wanted row j < m.  slot[j] < W (checked on the host), row_off has W + 1 entries; a row of one window holds fewer than 2^32 hashes
__global__ __launch_bounds__(256) void k_ro_lens(const uint64_t *__restrict__ row_off, const uint32_t *__restrict__ slot, uint64_t m, uint32_t *__restrict__ len) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const uint32_t s = slot[j];
    len[j] = (uint32_t)(row_off[s + 1] - row_off[s]);
}

// ---- gather: wavefront per taken row j < t.  Reads val[row_off[s] .. row_off[s + 1]) (k_rw_bounds: offsets ascend and end at n), writes
// blk[dst[j] .. dst[j + 1]) (dst[t] = the block's size) and entry k0 + j of the set's tables (k0 + t <= the tables' n_ids entries)
__global__ __launch_bounds__(256) void k_ro_gather(const uint32_t *__restrict__ val, const uint64_t *__restrict__ row_off, const uint32_t *__restrict__ slot,
                                                   const uint64_t *__restrict__ dst, uint64_t t, uint32_t *__restrict__ blk, uint64_t k0,
                                                   const uint32_t **__restrict__ row_ptr, uint32_t *__restrict__ row_len) {
    const uint64_t j = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (j >= t) return;
    const uint32_t lane = threadIdx.x & 63u, s = slot[j];
    const uint64_t r0 = row_off[s], n = row_off[s + 1] - r0;
    uint32_t *d = blk + dst[j];
    for (uint64_t i = lane; i < n; i += FD_WAVE) d[i] = val[r0 + i];
    if (lane == 0) { row_ptr[k0 + j] = d; row_len[k0 + j] = (uint32_t)n; }
}

// the failure tail of the set's build: the stream's work may still write into the set's blocks, so it ends before they go back to the pool
static int rowset_failed(fdgpu_ctx *c, int rc, fdgpu_rowset *rs) {
    (void)hipStreamSynchronize(c->stream);
    fdgpu_rowset_destroy(rs);
    return rc;
}
#define RS_HIPCHK(c, rs, expr)                                                                                     \
    do {                                                                                                           \
        hipError_t _e = (expr);                                                                                    \
        if (_e != hipSuccess) {                                                                                    \
            (c)->err = std::string("index rowset: ") + #expr + " -> " + hipGetErrorString(_e);                    \
            (void)hipGetLastError();                                                                               \
            return rowset_failed(c, FDGPU_EHIP, rs);                                                               \
        }                                                                                                          \
    } while (0)

static int rowset_impl(fdgpu_ctx *c, const fdgpu_index *ix, const uint32_t *ids, uint64_t n_ids, uint64_t window, uint64_t max_hashes,
                       fdgpu_rowset **out, uint64_t *n_taken) {
    reset_timings(c);
    hipStream_t st = c->stream;
    if (!window) window = OV_WINDOW_DEFAULT;
    const uint64_t id_end = ix->first_id + ix->n_structures;
    fdgpu_rowset *rs = new (std::nothrow) fdgpu_rowset;
    if (!rs) FAIL(c, FDGPU_ENOMEM, "index rowset: out of host memory");
    rs->ctx = c;
    if (n_ids) {
        void *p = nullptr;
        RS_HIPCHK(c, rs, fd_index_block(c, n_ids * 8, &p, &rs->cap_ptr));
        rs->row_ptr = (const uint32_t **)p;
        RS_HIPCHK(c, rs, fd_index_block(c, n_ids * 4, &p, &rs->cap_len));
        rs->row_len = (uint32_t *)p;
        try { rs->h_len.reserve(n_ids); } catch (...) { c->err = "index rowset: out of host memory"; return rowset_failed(c, FDGPU_ENOMEM, rs); }
    }
    std::vector<uint32_t> slot;
    std::vector<uint64_t> dst;
    uint64_t k = 0;
    bool full = false;
    while (k < n_ids && !full) {
        const uint64_t lo = ids[k], hi = std::min<uint64_t>(lo + window, id_end);
        const uint64_t k1 = std::lower_bound(ids + k, ids + n_ids, hi, [](uint32_t a, uint64_t b) { return a < b; }) - ids, m = k1 - k;
        fd_rows_dev R;
        const int rc = fd_rows_device(c, ix, lo, hi, "index rowset", &R);
        if (rc != FDGPU_OK) return rowset_failed(c, rc, rs);
        slot.resize(m);
        dst.resize(m + 1);
        for (uint64_t j = 0; j < m; ++j) slot[j] = (uint32_t)(ids[k + j] - lo);
        RS_HIPCHK(c, rs, c->ws[WS_MISC0].ensure(m * 4));                       // slots
        RS_HIPCHK(c, rs, c->ws[WS_MISC1].ensure(m * 4));                       // lens
        RS_HIPCHK(c, rs, c->ws[WS_SEGOFF].ensure((m + 1) * 8));                // dst
        RS_HIPCHK(c, rs, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(m) * 8 + 64));
        RS_HIPCHK(c, rs, c->ws[WS_TOTAL].ensure(64));
        uint32_t *d_slot = c->ws[WS_MISC0].as<uint32_t>(), *d_len = c->ws[WS_MISC1].as<uint32_t>();
        uint64_t *d_dst = c->ws[WS_SEGOFF].as<uint64_t>();
        {
            StageTimer t(c, "rowset_scan", m * (4 + 16 + 4 + 4 + 8));
            RS_HIPCHK(c, rs, hipMemcpyAsync(d_slot, slot.data(), m * 4, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_ro_lens, dim3(fd_grid(m, 256)), dim3(256), 0, st, R.row_off, d_slot, m, d_len);
            fd_exclusive_scan<uint32_t>(d_len, m, d_dst, c->ws[WS_SCANTMP].as<uint64_t>(), c->ws[WS_TOTAL].as<uint64_t>(), st);
        }
        RS_HIPCHK(c, rs, hipGetLastError());
        RS_HIPCHK(c, rs, hipMemcpyAsync(dst.data(), d_dst, m * 8, hipMemcpyDeviceToHost, st));
        RS_HIPCHK(c, rs, hipMemcpyAsync(&dst[m], c->ws[WS_TOTAL].as<uint64_t>(), 8, hipMemcpyDeviceToHost, st));
        RS_HIPCHK(c, rs, hipStreamSynchronize(st));
        uint64_t t = 0;                                   // the budget rule: a prefix of the wanted rows, by their lengths alone
        for (; t < m; ++t) {
            const uint64_t L = dst[t + 1] - dst[t];
            if (max_hashes && k + t > 0 && rs->n_hashes + L > max_hashes) { full = true; break; }
            rs->n_hashes += L;
            rs->h_len.push_back((uint32_t)L);
        }
        if (t) {
            fdgpu_rowset::block b{nullptr, 0, dst[t]};
            RS_HIPCHK(c, rs, fd_index_block(c, std::max<uint64_t>(b.n, 1) * 4, &b.p, &b.cap));
            rs->blocks.push_back(b);
            StageTimer tm(c, "rowset_gather", b.n * 8 + t * (4 + 16 + 8 + 12));
            hipLaunchKernelGGL(k_ro_gather, dim3(fd_grid(t, 4)), dim3(256), 0, st, R.val, R.row_off, d_slot, d_dst, t, (uint32_t *)b.p, k, rs->row_ptr, rs->row_len);
        }
        RS_HIPCHK(c, rs, hipGetLastError());
        k += t;
    }
    RS_HIPCHK(c, rs, hipStreamSynchronize(st));      // the set is complete, and the context's workspaces free again, when the call returns
    rs->n_rows = k;
    *out = rs; *n_taken = k;
    return FDGPU_OK;
}

extern "C" int fdgpu_index_rowset(fdgpu_ctx *c, const fdgpu_index *ix, const uint32_t *ids, uint64_t n_ids, uint64_t window, uint64_t max_hashes,
                                  fdgpu_rowset **out, uint64_t *n_taken) { FD_LOCK(c);
    if (!c || !ix || !out || !n_taken) return FDGPU_EINVAL;
    *out = nullptr; *n_taken = 0;
    if (n_ids && !ids) FAIL(c, FDGPU_EINVAL, "index rowset: ids is NULL with n_ids > 0");
    if (n_ids > 0xffffffffull) FAIL(c, FDGPU_EINVAL, "index rowset: 2^32 or more ids");
    for (uint64_t k = 0; k < n_ids; ++k) {
        if (ids[k] < ix->first_id || ids[k] - ix->first_id >= ix->n_structures)
            FAIL(c, FDGPU_EINVAL, "index rowset: id " + std::to_string(ids[k]) + " is outside [first_id, first_id + n_structures)");
        if (k && ids[k] <= ids[k - 1]) FAIL(c, FDGPU_EINVAL, "index rowset: the ids do not ascend strictly at position " + std::to_string(k));
    }
    return rowset_impl(c, ix, ids, n_ids, window, max_hashes, out, n_taken);
}

extern "C" int fdgpu_rowset_export(fdgpu_ctx *c, const fdgpu_rowset *rs, uint32_t **hashes, uint64_t **row_off) { FD_LOCK(c);
    if (!c || !rs || !hashes || !row_off) return FDGPU_EINVAL;
    *hashes = nullptr; *row_off = nullptr;
    if (rs->ctx != c) FAIL(c, FDGPU_EINVAL, "rowset export: the row set belongs to another context");
    uint32_t *h = (uint32_t *)fd_out_alloc(std::max<uint64_t>(rs->n_hashes, 1) * 4);
    uint64_t *ro = (uint64_t *)fd_out_alloc((rs->n_rows + 1) * 8);
    if (!h || !ro) { fdgpu_free(h); fdgpu_free(ro); FAIL(c, FDGPU_ENOMEM, "rowset export: out of host memory"); }
    ro[0] = 0;
    for (uint64_t k = 0; k < rs->n_rows; ++k) ro[k + 1] = ro[k] + rs->h_len[k];
    hipError_t e = hipSuccess;
    uint64_t at = 0;
    for (const auto &b : rs->blocks) {                // the blocks in window order are the rows in slot order
        if (b.n && e == hipSuccess) e = fd_d2h_big(c, h + at, b.p, b.n * 4);
        at += b.n;
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) { fdgpu_free(h); fdgpu_free(ro); c->err = std::string("rowset export: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    *hashes = h; *row_off = ro;
    return FDGPU_OK;
}

// ---- plan: thread per pair p < P.  ka[p] / kb[p] are row slots of their sets (checked on the host).  key = leading zeros of the pair's
// work + 1, less 30 (two rows of fewer than 2^32 hashes: work + 1 < 2^34), so 0 .. 33 and the smaller the longer
__global__ __launch_bounds__(256) void k_ov_plan(const uint32_t *__restrict__ len_a, const uint32_t *__restrict__ len_b, const uint32_t *__restrict__ ka,
                                                 const uint32_t *__restrict__ kb, uint64_t P, uint32_t *__restrict__ key, uint32_t *__restrict__ idx) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const unsigned long long work = (unsigned long long)len_a[ka[p]] + len_b[kb[p]] + 1ull;
    key[p] = (uint32_t)__clzll((long long)work) - 30u;
    idx[p] = (uint32_t)p;
}

// elements at .. at + 63 of a row of n: lane i gets element at + i, 0 past the end (the caller masks by length, the 0 is never compared)
__device__ __forceinline__ uint32_t ov_tile(const uint32_t *__restrict__ r, uint32_t n, uint64_t at, uint32_t lane) {
    return at + lane < n ? r[at + lane] : 0u;
}

// ---- pairs: wavefront per pair, in the order of `order`.  Reads row ka[p] of A and kb[p] of B inside their lengths only; writes inter[p]
__global__ __launch_bounds__(256) void k_ov_pairs(const uint32_t *const *__restrict__ ptr_a, const uint32_t *__restrict__ len_a,
                                                  const uint32_t *const *__restrict__ ptr_b, const uint32_t *__restrict__ len_b,
                                                  const uint32_t *__restrict__ ka, const uint32_t *__restrict__ kb, const uint32_t *__restrict__ order,
                                                  uint64_t P, uint32_t *__restrict__ inter) {
    __shared__ uint32_t tiles[4][OV_TILE];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t g = (uint64_t)blockIdx.x * 4u + wv;
    if (g >= P) return;
    const uint32_t p = order[g], sa = ka[p], sb = kb[p];
    const uint32_t *__restrict__ a = ptr_a[sa], *__restrict__ b = ptr_b[sb];
    const uint32_t na = len_a[sa], nb = len_b[sb];
    uint32_t *tb = tiles[wv];
    uint32_t ia = 0, ib = 0, hits = 0;
    uint32_t va = ov_tile(a, na, 0, lane), vb = ov_tile(b, nb, 0, lane);
    uint32_t pa = ov_tile(a, na, OV_TILE, lane), pb = ov_tile(b, nb, OV_TILE, lane);      // the tiles after the current ones, on their way
    bool new_b = true;
    while (ia < na && ib < nb) {                      // uniform over the wavefront
        const uint32_t ca = min(OV_TILE, na - ia), cb = min(OV_TILE, nb - ib);
        if (new_b) {
            fd_wave_lds_fence();                      // the lookups of the tile before are done
            tb[lane] = vb;
            fd_wave_lds_fence();
        }
        const uint32_t last_a = __shfl(va, (int)ca - 1, FD_WAVE), last_b = __shfl(vb, (int)cb - 1, FD_WAVE);
        uint32_t lo = 0, hi = cb;                     // tb[0 .. lo) < va <= tb[hi .. cb)
#pragma unroll
        for (int s = 0; s < 7; ++s) {                 // 2^7 > 64 + 1: the range is empty afterwards
            if (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (tb[mid] < va) lo = mid + 1; else hi = mid;
            }
        }
        const bool hit = lane < ca && lo < cb && tb[min(lo, OV_TILE - 1u)] == va;
        hits += (uint32_t)__popcll(__ballot(hit));
        const bool adv_a = last_a <= last_b;
        new_b = last_b <= last_a;
        if (adv_a) { ia += ca; va = pa; pa = ov_tile(a, na, (uint64_t)ia + OV_TILE, lane); }
        if (new_b) { ib += cb; vb = pb; pb = ov_tile(b, nb, (uint64_t)ib + OV_TILE, lane); }
    }
    if (lane == 0) inter[p] = hits;
}

static int intersect_impl(fdgpu_ctx *c, const fdgpu_rowset *A, const fdgpu_rowset *B, const uint32_t *ka, const uint32_t *kb, uint64_t P, uint32_t **out) {
    reset_timings(c);
    hipStream_t st = c->stream;
    uint32_t *res = (uint32_t *)fd_out_alloc(std::max<uint64_t>(P, 1) * 4);
    if (!res) FAIL(c, FDGPU_ENOMEM, "rowset intersect: out of host memory");
    res[0] = 0;
    if (!P) { *out = res; return FDGPU_OK; }
    const size_t kbytes = P * 4;
    hipError_t e = hipSuccess;
    auto need = [&](int w, size_t bytes) { if (e == hipSuccess) e = c->ws[w].ensure(bytes); };
    need(WS_MISC0, 2 * kbytes);                                       // the pairs' slots
    need(WS_MISC5, kbytes);                                           // the result
    need(WS_KEYS_A, kbytes); need(WS_IDS_A, kbytes + 16);             // the sizes of the build's sort buffers (ensure_sort_ws)
    need(WS_KEYS_B, kbytes); need(WS_IDS_B, kbytes + 16);
    need(WS_GHIST, (size_t)256 * std::max<uint32_t>(fd_rs_num_tiles(P), 1) * 4);
    need(WS_TOT, (256 + (size_t)(fd_rs_num_tiles(P) / 128 + 2) * 256) * 8);
    if (e == hipSuccess) {
        uint32_t *d_ka = c->ws[WS_MISC0].as<uint32_t>(), *d_kb = d_ka + P, *d_res = c->ws[WS_MISC5].as<uint32_t>();
        uint32_t *key_a = c->ws[WS_KEYS_A].as<uint32_t>(), *idx_a = c->ws[WS_IDS_A].as<uint32_t>();
        uint32_t *key_b = c->ws[WS_KEYS_B].as<uint32_t>(), *idx_b = c->ws[WS_IDS_B].as<uint32_t>();
        {
            StageTimer t(c, "overlap_upload", 2 * kbytes);
            e = hipMemcpyAsync(d_ka, ka, kbytes, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(d_kb, kb, kbytes, hipMemcpyHostToDevice, st);
        }
        if (e == hipSuccess) {
            {
                StageTimer t(c, "overlap_plan", P * (8 + 8 + 8));
                hipLaunchKernelGGL(k_ov_plan, dim3(fd_grid(P, 256)), dim3(256), 0, st, A->row_len, B->row_len, d_ka, d_kb, P, key_a, idx_a);
            }
            const uint32_t *order = sort_pairs(c, key_a, idx_a, key_b, idx_b, P, OV_KEY_BITS) ? idx_b : idx_a;
            {
                StageTimer t(c, "overlap_pairs", P * (4 + 8 + 2 * 12 + 4));      // + the rows' bytes, which depend on their values
                hipLaunchKernelGGL(k_ov_pairs, dim3(fd_grid(P, 4)), dim3(256), 0, st, A->row_ptr, A->row_len, B->row_ptr, B->row_len, d_ka, d_kb, order, P, d_res);
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            StageTimer t(c, "overlap_copy", kbytes);
            e = fd_d2h_big(c, res, d_res, kbytes);
        }
    }
    const hipError_t es = hipStreamSynchronize(st);      // the result is complete, and nothing of a failed call still runs, when the call returns
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fdgpu_free(res);
        c->err = std::string("rowset intersect: ") + hipGetErrorString(e);
        return FDGPU_EHIP;
    }
    *out = res;
    return FDGPU_OK;
}

extern "C" int fdgpu_rowset_intersect(fdgpu_ctx *c, const fdgpu_rowset *A, const fdgpu_rowset *B, const uint32_t *ka, const uint32_t *kb,
                                      uint64_t n_pairs, uint32_t **inter) { FD_LOCK(c);
    if (!c || !A || !inter) return FDGPU_EINVAL;
    *inter = nullptr;
    if (!B) B = A;
    if (A->ctx != c || B->ctx != c) FAIL(c, FDGPU_EINVAL, "rowset intersect: a row set belongs to another context");
    if (n_pairs && (!ka || !kb)) FAIL(c, FDGPU_EINVAL, "rowset intersect: ka or kb is NULL with n_pairs > 0");
    if (n_pairs > 0xffffffffull) FAIL(c, FDGPU_EINVAL, "rowset intersect: 2^32 or more pairs");
    for (uint64_t p = 0; p < n_pairs; ++p)
        if (ka[p] >= A->n_rows || kb[p] >= B->n_rows)
            FAIL(c, FDGPU_EINVAL, "rowset intersect: pair " + std::to_string(p) + " names a row slot at or above its set's row count");
    return intersect_impl(c, A, B, ka, kb, n_pairs, inter);
}
