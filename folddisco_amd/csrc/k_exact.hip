// k_exact.hip — exact neighbours (fdgpu_rowset_neighbors): for every row of a row set its k nearest structures of a resident index by the Jaccard
// similarity of the rows; the definition is include/fdgpu.h, the predicate and the order fd_row_neighbor.h, the host form
// fd_neighbors_exact_host.cpp, the account DESIGN.md §4k.
//
// The index is the data structure: the structures that share a hash with a query row R_q are the ids in the posting lists of R_q's hashes,
// and the number of those lists that hold s is |R_q ∩ R_s|.  The queries go in blocks of QB rows, each block with a u32 counter table
// cnt[QB][S] (zero between the blocks):
//   k_xn_count   wavefront per (query row, chunk of 64 of its hashes); the chunk table comes from the set's host-side lengths.  Every lane
//                looks its hash up in D's sorted hash table by bisection and gets the list's byte range; the wavefront then takes the 64
//                ranges in turn (readlane) and walks each 256 bytes a step (fd_wave_walk): every decoded id is tested with fd_id_local — an
//                id outside D raises the damaged flag and is never used as an address — and then counted with a no-return atomic add
//   k_xn_select  grid (query of the block, split of the id range), one wavefront each: the lanes stride the split's counters (read once,
//                a non-zero one written back as zero), apply the candidate test and insert into a per-lane k-list in LDS ([slot][lane], as
//                k_sg_near); the wavefront merges its 64 sorted lists by taking the nearest head k times
//   k_xn_merge   only with several splits: a wavefront per query takes the nearest head of the splits' sorted lists k times
// Integer adds commute, so the table is the same from run to run; the order is total, so the selection does not depend on which lane or
// split met a candidate.  The adds are scattered over S — see DESIGN.md §4k for what that costs and for the shaped alternative.
// Workspace: 4 * QB * S (counters) + 4 * S (d_len) + 4 * nQ (exclude) + 8 per chunk + 16 * k per query and split.
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>
#include "fdgpu_internal.h"
#include "fd_api_common.h"
#include "fd_postings.h"
#include "fd_row_neighbor.h"

#define XN_DEFAULT_COUNTER_BYTES ((uint64_t)1 << 30)
#define XN_MAX_SPLIT 64u          // lists a merging wavefront takes, one per lane
#define XN_ERR_LENGTHS 4u         // beside FD_IXERR_*: a counter above min(|R_q|, d_len)

struct xn_count_args {
    const uint32_t *const *row_ptr; const uint32_t *row_len;                    // the query set
    const uint32_t *hashes; const uint64_t *offsets; const uint8_t *value;      // D
    uint64_t H, value_len, S; uint32_t first_id;
    const uint2 *chunks; uint64_t n_chunks;                                     // {row slot, first element} of every chunk of the block
    uint32_t q0;                                                                // the block's first row slot
    uint32_t *cnt, *err;
};

__device__ __forceinline__ uint64_t xn_readlane64(uint64_t v, uint32_t l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return (uint64_t)hi << 32 | lo;
}

// ---- count: wavefront per chunk g < n_chunks.  Reads elements at .. at + 63 of row q inside its length, hashes[0 .. H), offsets[0 .. H],
// the value bytes of sound ranges only (b0 < b1 <= value_len; FD_VALUE_SLACK behind them); adds to cnt[(q - q0) * S + loc] for loc < S only
__global__ __launch_bounds__(256) void k_xn_count(xn_count_args A) {
    const uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= A.n_chunks) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint2 ch = A.chunks[g];
    const uint32_t q = ch.x, at = ch.y, n_in = min(64u, A.row_len[q] - at);
    uint64_t b0 = 0, b1 = 0;      // the lane's list; an absent hash, a lane beyond the chunk and a damaged range: empty
    bool bad = false;
    if (lane < n_in) {
        const uint32_t h = A.row_ptr[q][at + lane];
        uint64_t lo = 0, hi = A.H;      // hashes below lo are < h, hashes from hi on are >= h
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (A.hashes[mid] < h) lo = mid + 1; else hi = mid;
        }
        if (lo < A.H && A.hashes[lo] == h) {
            const uint64_t x0 = A.offsets[lo], x1 = A.offsets[lo + 1];
            if (x1 <= x0 || x1 > A.value_len || (A.value[x1 - 1] & 0x80u)) bad = true;
            else { b0 = x0; b1 = x1; }
        }
    }
    uint32_t *__restrict__ row = A.cnt + (uint64_t)(q - A.q0) * A.S;
    for (uint32_t l = 0; l < n_in; ++l) {      // uniform over the wavefront
        const uint64_t w0 = xn_readlane64(b0, l), w1 = xn_readlane64(b1, l);
        if (w0 >= w1) continue;
        fd_wave_walk(A.value, w0, w1, lane, [&](const fd_step &ds, uint32_t id0) {
            fd_lane_starts(ds, id0, [&](uint32_t j, uint32_t id) {
                uint64_t loc;
                // no end in five bytes, or a fifth byte with more than four value bits; an id that is not D's: flagged, never an address
                if (ds.nf[j] == 0 || (ds.nf[j] == 5 && ((uint32_t)(ds.win >> (8u * j + 32u)) & 0x70u)) || !fd_id_local(id, A.first_id, A.S, &loc)) bad = true;
                else (void)atomicAdd(row + loc, 1u);
            });
        });
    }
    if (bad) atomicOr(A.err, FD_IXERR_DAMAGED);
}

struct xn_select_args {
    const uint32_t *row_len, *d_len, *excl;      // excl: per row slot of the set, or null
    uint32_t *cnt, *err;
    uint64_t S; uint32_t first_id, q0, nb, k, T, tiles_per_split;
    uint4 *part;                                 // [split][query of the block][k]
};

// the nearest of the wavefront's 64 heads, the same in every lane: the lists hold different candidates, so the order is strict until only
// empty slots are left, and those are equal in every word
__device__ __forceinline__ void xn_wave_nearest(uint32_t &id, uint32_t &in, uint32_t &un, uint32_t &fl, uint32_t &src) {
    for (int o = FD_WAVE / 2; o > 0; o >>= 1) {
        const uint32_t oid = __shfl_xor(id, o, FD_WAVE), oin = __shfl_xor(in, o, FD_WAVE), oun = __shfl_xor(un, o, FD_WAVE), ofl = __shfl_xor(fl, o, FD_WAVE),
                       osrc = __shfl_xor(src, o, FD_WAVE);
        if (fd_row_nearer(oin, oun, oid, in, un, id)) { id = oid; in = oin; un = oun; fl = ofl; src = osrc; }
    }
}

// ---- select: one wavefront per (query ql < nb, split).  Reads and clears cnt[ql * S + loc] for the split's loc < S, reads d_len[loc];
// writes part[(split * nb + ql) * k + 0 .. k).  Dynamic LDS: k * 768 bytes, slot s of the lane's list at [s * 64 + lane] in three planes
__global__ __launch_bounds__(64) void k_xn_select(xn_select_args P) {
    extern __shared__ uint32_t xn_lds[];
    const uint32_t lane = threadIdx.x, K = P.k, ql = blockIdx.x;
    uint32_t *l_id = xn_lds + lane, *l_in = l_id + K * FD_WAVE, *l_un = l_in + K * FD_WAVE;
    const uint32_t len_q = P.row_len[P.q0 + ql], skip = P.excl ? P.excl[P.q0 + ql] : FD_ROW_NO_ID;
    for (uint32_t s = 0; s < K; ++s) { l_id[s * FD_WAVE] = FD_ROW_NO_ID; l_in[s * FD_WAVE] = 0u; l_un[s * FD_WAVE] = 0u; }
    uint32_t kth_id = FD_ROW_NO_ID, kth_in = 0u, kth_un = 0u;      // the list's last slot: what a candidate has to beat
    uint32_t *__restrict__ row = P.cnt + (uint64_t)ql * P.S;
    const uint64_t lo = (uint64_t)blockIdx.y * P.tiles_per_split * FD_WAVE, hi = min(P.S, lo + (uint64_t)P.tiles_per_split * FD_WAVE);
    bool bad = false;
    for (uint64_t base = lo; base < hi; base += 4u * FD_WAVE) {
        uint32_t c[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {             // four counters on their way before the first is looked at
            const uint64_t loc = base + u * FD_WAVE + lane;
            c[u] = loc < hi ? row[loc] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            if (!c[u]) continue;
            const uint64_t loc = base + u * FD_WAVE + lane;
            row[loc] = 0u;                             // clean for the next block
            const uint32_t inter = c[u], dl = P.d_len[loc], id = P.first_id + (uint32_t)loc;
            if (inter > min(len_q, dl)) { bad = true; continue; }
            const uint32_t uni = len_q + dl - inter;
            if (id == skip || !fd_row_candidate(inter, uni, P.T) || !fd_row_nearer(inter, uni, id, kth_in, kth_un, kth_id)) continue;
            uint32_t a = 0, b = K - 1;                 // its slot: the first one it is nearer than (the last one at the latest), by bisection
            while (a < b) {
                const uint32_t mid = (a + b) >> 1;
                if (fd_row_nearer(inter, uni, id, l_in[mid * FD_WAVE], l_un[mid * FD_WAVE], l_id[mid * FD_WAVE])) b = mid; else a = mid + 1;
            }
            for (uint32_t s = K - 1; s > a; --s) {     // the slots from there on move down by one, the last one leaves
                l_id[s * FD_WAVE] = l_id[(s - 1u) * FD_WAVE]; l_in[s * FD_WAVE] = l_in[(s - 1u) * FD_WAVE]; l_un[s * FD_WAVE] = l_un[(s - 1u) * FD_WAVE];
            }
            l_id[a * FD_WAVE] = id; l_in[a * FD_WAVE] = inter; l_un[a * FD_WAVE] = uni;
            kth_id = l_id[(K - 1) * FD_WAVE]; kth_in = l_in[(K - 1) * FD_WAVE]; kth_un = l_un[(K - 1) * FD_WAVE];
        }
    }
    if (bad) atomicOr(P.err, XN_ERR_LENGTHS);
    // the 64 sorted lists -> the wavefront's k nearest; every lane reads its own column only, so no barrier
    uint4 *out = P.part + ((uint64_t)blockIdx.y * P.nb + ql) * K;
    uint32_t pos = 0, h_id = l_id[0], h_in = l_in[0], h_un = l_un[0];
    for (uint32_t r = 0; r < K; ++r) {
        uint32_t id = h_id, in = h_in, un = h_un, fl = 0u, src = lane;
        xn_wave_nearest(id, in, un, fl, src);
        if (lane == 0) out[r] = make_uint4(id, in, un, fd_row_flags(id, in, un, len_q));
        if (src == lane && id != FD_ROW_NO_ID) {
            ++pos;
            h_id = pos < K ? l_id[pos * FD_WAVE] : FD_ROW_NO_ID; h_in = pos < K ? l_in[pos * FD_WAVE] : 0u; h_un = pos < K ? l_un[pos * FD_WAVE] : 0u;
        }
    }
}

// ---- merge: a wavefront per query ql < nb; lane l < splits owns the sorted list part[(l * nb + ql) * k + 0 .. k); k times the wavefront takes
// the nearest head and the lane it came from steps on.  Writes out[ql * k + 0 .. k)
__global__ __launch_bounds__(256) void k_xn_merge(const uint4 *__restrict__ part, uint32_t splits, uint32_t nb, uint32_t k, uint4 *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t ql = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (ql >= nb) return;
    const uint4 none = make_uint4(FD_ROW_NO_ID, 0u, 0u, 0u);
    const uint4 *src_list = part + ((uint64_t)(lane < splits ? lane : 0u) * nb + ql) * k;
    uint32_t pos = 0;
    uint4 head = lane < splits ? src_list[0] : none;
    for (uint32_t r = 0; r < k; ++r) {
        uint32_t id = head.x, in = head.y, un = head.z, fl = head.w, src = lane;
        xn_wave_nearest(id, in, un, fl, src);
        if (lane == 0) out[ql * k + r] = make_uint4(id, in, un, fl);
        if (src == lane && id != FD_ROW_NO_ID) { ++pos; head = pos < k ? src_list[pos] : none; }
    }
}

static int neighbors_impl(fdgpu_ctx *c, const fdgpu_rowset *Q, const fdgpu_index *D, const uint32_t *d_len, const uint32_t *exclude, uint32_t k, uint32_t T,
                          uint64_t max_counter_bytes, fd_row_neighbor **out) {
    reset_timings(c);
    hipStream_t st = c->stream;
    const uint64_t nQ = Q->n_rows, S = D->n_structures, n_rec = nQ * k;
    fd_row_neighbor *res = (fd_row_neighbor *)fd_out_alloc(std::max<uint64_t>(n_rec, 1) * sizeof(fd_row_neighbor));
    if (!res) FAIL(c, FDGPU_ENOMEM, "rowset neighbors: out of host memory");
    const fd_row_neighbor none = {FD_ROW_NO_ID, 0, 0, 0};
    if (!nQ || !S || !D->n_hashes || !Q->n_hashes) {      // nothing to count: every slot is empty
        for (uint64_t i = 0; i < std::max<uint64_t>(n_rec, 1); ++i) res[i] = none;
        *out = res;
        return FDGPU_OK;
    }
    if (!max_counter_bytes) max_counter_bytes = XN_DEFAULT_COUNTER_BYTES;
    const uint64_t QB = std::max<uint64_t>(1, std::min<uint64_t>(max_counter_bytes / (4 * S), nQ));
    const uint32_t tiles = fd_grid(S, FD_WAVE), most = std::min<uint32_t>(tiles, XN_MAX_SPLIT);
    // enough wavefronts to fill the device, no more splits than tiles; FDGPU_XN_SPLIT (tests) moves the boundary
    uint32_t splits = std::max<uint32_t>(1u, std::min<uint32_t>(most, fd_grid(8192, QB)));
    if (const char *e = getenv("FDGPU_XN_SPLIT")) {
        const long long v = atoll(e);
        if (v > 0) splits = (uint32_t)std::min<long long>(v, most);
    }
    const uint32_t tiles_per_split = fd_grid(tiles, splits);
    std::vector<uint2> chunks;                            // per query in order: {row slot, first element} of every 64 hashes
    std::vector<uint64_t> chunk0(nQ + 1, 0);
    try {
        for (uint64_t q = 0; q < nQ; ++q) {
            for (uint64_t at = 0; at < Q->h_len[q]; at += FD_WAVE) chunks.push_back(make_uint2((uint32_t)q, (uint32_t)at));
            chunk0[q + 1] = chunks.size();
        }
    } catch (...) { fdgpu_free(res); FAIL(c, FDGPU_ENOMEM, "rowset neighbors: out of host memory"); }
    // the byte column of xn_count is NOMINAL: the index's value bytes once per block, not the bytes the block's queries walk (those depend on
    // which lists they name and are not known on the host; tools/exact_neighbors_probe.py derives the postings walked from the list lengths)
    const uint64_t postings_bytes = D->value_len;
    uint32_t flags = 0;
    hipError_t e = hipSuccess;
    do {
        if ((e = c->ws[WS_XN_CNT].ensure(QB * S * 4)) != hipSuccess) break;
        if ((e = c->ws[WS_XN_OUT].ensure(n_rec * sizeof(fd_row_neighbor))) != hipSuccess) break;
        if (splits > 1 && (e = c->ws[WS_XN_PART].ensure((uint64_t)splits * QB * k * sizeof(fd_row_neighbor))) != hipSuccess) break;
        if ((e = c->ws[WS_MISC0].ensure(chunks.size() * sizeof(uint2))) != hipSuccess) break;
        if ((e = c->ws[WS_MISC1].ensure(S * 4)) != hipSuccess) break;
        if (exclude && (e = c->ws[WS_MISC2].ensure(nQ * 4)) != hipSuccess) break;
        if ((e = c->ws[WS_TOTAL].ensure(64)) != hipSuccess) break;
        uint32_t *cnt = c->ws[WS_XN_CNT].as<uint32_t>(), *d_dlen = c->ws[WS_MISC1].as<uint32_t>(), *d_err = c->ws[WS_TOTAL].as<uint32_t>();
        uint32_t *d_excl = exclude ? c->ws[WS_MISC2].as<uint32_t>() : nullptr;
        uint2 *d_chunks = c->ws[WS_MISC0].as<uint2>();
        uint4 *d_out = c->ws[WS_XN_OUT].as<uint4>();
        {
            StageTimer t(c, "xn_upload", chunks.size() * sizeof(uint2) + S * 4 + (exclude ? nQ * 4 : 0) + QB * S * 4);
            if ((e = hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * sizeof(uint2), hipMemcpyHostToDevice, st)) != hipSuccess) break;
            if ((e = hipMemcpyAsync(d_dlen, d_len, S * 4, hipMemcpyHostToDevice, st)) != hipSuccess) break;
            if (exclude && (e = hipMemcpyAsync(d_excl, exclude, nQ * 4, hipMemcpyHostToDevice, st)) != hipSuccess) break;
            if ((e = hipMemsetAsync(d_err, 0, 64, st)) != hipSuccess) break;
            if ((e = hipMemsetAsync(cnt, 0, QB * S * 4, st)) != hipSuccess) break;      // the select leaves it zero for the next block
        }
        const size_t lds = (size_t)k * 3u * FD_WAVE * 4u;
        for (uint64_t q0 = 0; q0 < nQ && e == hipSuccess; q0 += QB) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(QB, nQ - q0);
            const uint64_t c0 = chunk0[q0], n_chunks = chunk0[q0 + nb] - c0;
            uint4 *d_part = splits > 1 ? c->ws[WS_XN_PART].as<uint4>() : d_out + q0 * k;
            if (n_chunks) {
                StageTimer t(c, "xn_count", n_chunks * (8 + 64 * 4) + postings_bytes);
                const xn_count_args A{Q->row_ptr, Q->row_len, D->hashes, D->offsets, D->value, D->n_hashes, D->value_len, S, (uint32_t)D->first_id,
                                      d_chunks + c0, n_chunks, (uint32_t)q0, cnt, d_err};
                hipLaunchKernelGGL(k_xn_count, dim3(fd_grid(n_chunks, 4)), dim3(256), 0, st, A);
            }
            {
                StageTimer t(c, "xn_select", (uint64_t)nb * S * 4 + (uint64_t)nb * splits * k * sizeof(fd_row_neighbor));
                const xn_select_args P{Q->row_len, d_dlen, d_excl, cnt, d_err, S, (uint32_t)D->first_id, (uint32_t)q0, nb, k, T, tiles_per_split, d_part};
                hipLaunchKernelGGL(k_xn_select, dim3(nb, splits), dim3(64), lds, st, P);
            }
            if (splits > 1) {
                StageTimer t(c, "xn_merge", ((uint64_t)splits + 1) * nb * k * sizeof(fd_row_neighbor));
                hipLaunchKernelGGL(k_xn_merge, dim3(fd_grid(nb, 4)), dim3(256), 0, st, d_part, splits, nb, k, d_out + q0 * k);
            }
            e = hipGetLastError();
        }
        if (e != hipSuccess) break;
        {
            StageTimer t(c, "xn_copy", n_rec * sizeof(fd_row_neighbor) + 4);
            if ((e = hipMemcpyAsync(&flags, d_err, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) break;
            e = fd_d2h_big(c, res, d_out, n_rec * sizeof(fd_row_neighbor));
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    } while (false);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);                   // nothing of a failed call still writes into the block
        (void)hipGetLastError();
        fdgpu_free(res);
        c->err = std::string("rowset neighbors: ") + hipGetErrorString(e);
        return FDGPU_EHIP;
    }
    if (flags) {
        fdgpu_free(res);
        if (flags & FD_IXERR_DAMAGED)
            FAIL(c, FDGPU_EINVAL, "rowset neighbors: the index is damaged (offsets that do not ascend inside the value bytes, a varint that leaves its list, "
                                  "or ids outside [first_id, first_id + n_structures))");
        FAIL(c, FDGPU_EINVAL, "rowset neighbors: row lengths do not belong to this index (a structure shares more hashes with a query than d_len gives its row)");
    }
    *out = res;
    return FDGPU_OK;
}

extern "C" int fdgpu_rowset_neighbors(fdgpu_ctx *c, const fdgpu_rowset *Q, const fdgpu_index *D, const uint32_t *d_len, const uint32_t *exclude, uint32_t k,
                                      uint32_t floor_e4, uint64_t max_counter_bytes, fd_row_neighbor **out) { FD_LOCK(c);
    if (!c || !out) return FDGPU_EINVAL;
    *out = nullptr;
    if (!Q || !D) FAIL(c, FDGPU_EINVAL, "rowset neighbors: the row set or the index is NULL");
    if (Q->ctx != c) FAIL(c, FDGPU_EINVAL, "rowset neighbors: the row set belongs to another context");
    if (k < 1 || k > FD_ROW_MAX_K) FAIL(c, FDGPU_EINVAL, "rowset neighbors: k must be 1 .. 32");
    if (floor_e4 > FD_ROW_FLOOR_MAX) FAIL(c, FDGPU_EINVAL, "rowset neighbors: floor_e4 must be 0 .. 10000");
    if (D->n_structures && !d_len) FAIL(c, FDGPU_EINVAL, "rowset neighbors: d_len is NULL with structures in the index");
    if (D->first_id + D->n_structures > 0xffffffffull) FAIL(c, FDGPU_EINVAL, "rowset neighbors: the index's ids leave 32 bits");
    if (exclude)
        for (uint64_t q = 0; q < Q->n_rows; ++q)
            if (exclude[q] != FD_ROW_NO_ID && (exclude[q] < D->first_id || exclude[q] - D->first_id >= D->n_structures))
                FAIL(c, FDGPU_EINVAL, "rowset neighbors: exclude[" + std::to_string(q) + "] is neither 0xFFFFFFFF nor an id of the index");
    return neighbors_impl(c, Q, D, d_len, exclude, k, floor_e4, max_counter_bytes, out);
}
