// k_prune.hip — device-side removal of structures from a resident index (fdgpu_index_remove).
//
// Removing structures renumbers every later id densely (kept structures keep their order), so the result must equal a fresh build over the
// kept structures byte for byte.  Per posting list (first id f, last id l, ids absolute at the head, deltas behind it, LEB128 varints):
//
//   removed id in [f, l]                 RE-ENCODE: decode, drop the removed ids, remap the kept ones, re-delta, re-varint
//   none in [f, l], some below f         RE-BASE: only the absolute head changes (new id of f), the rest moves verbatim (the head re-base of
//                                        k_mg_sizes / k_mg_copy)
//   none at or below l                   VERBATIM copy
//
// The new id of a kept structure x is first_id + K[x], K = exclusive prefix count of the keep mask (one scan); "removed ids in [f, l]" is
// (l - f + 1) - (K[l + 1] - K[f]).  Lists that lose every id get size 0 and drop out of the sparse hash table with their hash.
//
//   k_pr_plan       thread per list: head, last id, mode, new size of RE-BASE / VERBATIM lists, long-first order key
//   order           re-encoded lists in the order the decode kernels take them, lists of FD_LONG_LIST_BYTES and more first (fd_order_long_first,
//                   shared with k_split.hip and k_permute.hip)
//   k_pr_recode<W>  wavefront per re-encoded list, 256 bytes per step (four per lane; fd_wave_walk of fd_postings.h, shared with k_split.hip
//                   and k_permute.hip): terminator bits -> varint starts, each start decodes from the lane's and its neighbour's word, wave
//                   scans turn deltas into ids and place the new deltas; W = 0 sizes, W = 1 writes
//   k_pr_copy       eight lanes per RE-BASE / VERBATIM list, 16 bytes per lane and step, new head first
//   k_pr_compact    hashes / offsets / last ids of the non-empty lists at their new slots
// HBM-bound byte work: the value bytes are read twice (sizes, write) and written once; 8 bytes per hash of tables.
#include "fdgpu_internal.h"
#include "fd_api_common.h"
#include "fd_postings.h"

#define PR_MODE_COPY 0u
#define PR_MODE_REBASE 1u
#define PR_MODE_RECODE 2u

struct pr_args {
    const uint64_t *offsets; const uint8_t *value; const uint32_t *last_ids; uint64_t H;
    const uint64_t *K; uint64_t S; uint32_t first_id;
};

// ---- plan: thread per list
__global__ __launch_bounds__(256) void k_pr_plan(pr_args A, uint32_t *__restrict__ sizes, uint32_t *__restrict__ new_last, uint8_t *__restrict__ mode,
                                                 uint8_t *__restrict__ recode, uint8_t *__restrict__ is_long, uint32_t *__restrict__ err) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.H) return;
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    uint32_t nf = 0;
    const uint32_t f = fd_first_varint(A.value + b0, &nf), l = A.last_ids[t];
    const uint64_t fl = (uint64_t)f - A.first_id, ll = (uint64_t)l - A.first_id;
    uint32_t m = PR_MODE_COPY, sz = (uint32_t)(b1 - b0), nl = l;
    if (b1 - b0 > 0xffffffffull) atomicOr(err, FD_IXERR_LONG);           // a list of 4 GiB or more: FDGPU_ERANGE
    if (b1 <= b0 || f < A.first_id || l < f || ll >= A.S) {
        atomicOr(err, FD_IXERR_DAMAGED);                                 // an id outside [first_id, first_id + S): the index does not match n_keep
        sz = 0;
    } else {
        const uint64_t removed = (ll - fl + 1) - (A.K[ll + 1] - A.K[fl]);
        if (removed) m = PR_MODE_RECODE;
        else {
            const uint32_t nfirst = A.first_id + (uint32_t)A.K[fl];
            nl = A.first_id + (uint32_t)A.K[ll];
            if (nfirst != f) { m = PR_MODE_REBASE; sz = sz - nf + fd_varint_len(nfirst); }
        }
    }
    sizes[t] = m == PR_MODE_RECODE ? 0u : sz;
    new_last[t] = nl;
    mode[t] = (uint8_t)m;
    recode[t] = m == PR_MODE_RECODE ? 1u : 0u;
    is_long[t] = (m == PR_MODE_RECODE && b1 - b0 >= FD_LONG_LIST_BYTES) ? 1u : 0u;
}

// ---- re-encode: wavefront per list, 64 lanes x 4 bytes per step.  W = false: new byte size, new last id, removed postings; W = true: new bytes.
template <bool W>
__global__ __launch_bounds__(256) void k_pr_recode(pr_args A, const uint32_t *__restrict__ order, uint64_t n_recode, uint32_t *__restrict__ sizes,
                                                   uint32_t *__restrict__ new_last, unsigned long long *__restrict__ removed_total,
                                                   const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out_value, uint32_t *__restrict__ err) {
    const uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= n_recode) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = order[g];
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    uint8_t *dst = W ? out_value + out_off[t] : nullptr;
    uint64_t prev_new = 0;        // new id + 1 of the last KEPT element so far, 0 = none yet
    uint32_t out_pos = 0, removed = 0;
    fd_wave_walk(A.value, b0, b1, lane, [&](const fd_step &ds, uint32_t id0) {      // id0: the OLD id before this lane's first element
        // keep / remap; the lane's last kept new id for the predecessor scan
        uint32_t nid[4] = {0, 0, 0, 0};
        uint32_t kmask = 0;
        uint64_t lane_last = 0;
        fd_lane_starts(ds, id0, [&](uint32_t j, uint32_t id) {
            uint64_t loc;
            if (!fd_id_local(id, A.first_id, A.S, &loc)) { atomicOr(err, FD_IXERR_DAMAGED); ++removed; return; }
            const uint64_t k0 = A.K[loc], k1 = A.K[loc + 1];      // kept iff the prefix count steps here: no dependent load of the mask
            if (k1 != k0) { nid[j] = A.first_id + (uint32_t)k0; kmask |= 1u << j; lane_last = (uint64_t)nid[j] + 1u; }
            else ++removed;
        });
        const uint64_t lmax = fd_wave_scan_max(lane_last, lane);
        uint64_t pred = __shfl_up(lmax, 1, FD_WAVE);      // new id + 1 of the last kept element before this lane (0: none)
        if (lane == 0) pred = 0;
        if (prev_new > pred) pred = prev_new;
        // new deltas and their lengths
        uint32_t nd[4], ln[4], lsum = 0;
        uint64_t q = pred;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            ln[j] = 0; nd[j] = 0;
            if ((kmask >> j) & 1u) {
                nd[j] = q ? nid[j] - (uint32_t)(q - 1u) : nid[j];
                ln[j] = fd_varint_len(nd[j]);
                lsum += ln[j];
                q = (uint64_t)nid[j] + 1u;
            }
        }
        const uint32_t linc = fd_wave_scan_add(lsum, lane);
        if (W) {
            uint8_t *o = dst + out_pos + (linc - lsum);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) { fd_varint_store(o, nd[j], ln[j]); o += ln[j]; }
        }
        // carries into the next step
        out_pos += __shfl(linc, FD_WAVE - 1, FD_WAVE);
        const uint64_t m63 = __shfl(lmax, FD_WAVE - 1, FD_WAVE);
        if (m63 > prev_new) prev_new = m63;
    });
    if (!W) {
        removed = fd_wave_sum(removed);
        if (lane == 0) {
            sizes[t] = out_pos;
            new_last[t] = prev_new ? (uint32_t)(prev_new - 1u) : 0u;
            if (removed) atomicAdd(removed_total, (unsigned long long)removed);
        }
    }
}

// ---- RE-BASE / VERBATIM lists: eight lanes per list (fd_list_copy), new head varint first, then the bytes behind the old head
__global__ __launch_bounds__(256) void k_pr_copy(pr_args A, const uint8_t *__restrict__ mode, const uint32_t *__restrict__ sizes,
                                                 const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out_value) {
    const uint64_t t = (uint64_t)blockIdx.x * 32u + (threadIdx.x >> 3);
    if (t >= A.H) return;
    const uint32_t m = mode[t];
    if (m == PR_MODE_RECODE || sizes[t] == 0) return;
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    const uint8_t *sp = A.value + b0;
    uint64_t n = b1 - b0;
    uint32_t head = 0, dl = 0;
    if (m == PR_MODE_REBASE) {
        uint32_t nf = 0;
        const uint32_t f = fd_first_varint(sp, &nf);
        head = A.first_id + (uint32_t)A.K[(uint64_t)f - A.first_id];
        dl = fd_varint_len(head);
        sp += nf; n -= nf;
    }
    fd_list_copy(out_value + out_off[t], head, dl, sp, n, threadIdx.x & 7u);
}

// ---- non-empty lists -> their slots; offsets[H'] = the new value length
__global__ void k_pr_compact(const uint32_t *__restrict__ hashes, const uint32_t *__restrict__ sizes, const uint32_t *__restrict__ new_last,
                             const uint64_t *__restrict__ slot, const uint64_t *__restrict__ off_all, uint64_t H, uint32_t *__restrict__ out_hashes,
                             uint64_t *__restrict__ out_offsets, uint32_t *__restrict__ out_last) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) out_offsets[slot[H]] = off_all[H];
    if (t >= H || sizes[t] == 0) return;
    const uint64_t s = slot[t];
    out_hashes[s] = hashes[t];
    out_offsets[s] = off_all[t];
    out_last[s] = new_last[t];
}
__global__ void k_pr_nonzero(const uint32_t *__restrict__ sizes, uint64_t H, uint8_t *__restrict__ flag) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < H) flag[t] = sizes[t] ? 1u : 0u;
}

extern "C" int fdgpu_index_remove(fdgpu_ctx *c, const fdgpu_index *ix, const uint8_t *keep, uint64_t n_keep, fdgpu_index **out) { FD_LOCK(c);
    if (!c || !ix || !out || (n_keep && !keep)) return FDGPU_EINVAL;
    *out = nullptr;
    if (n_keep != ix->n_structures) FAIL(c, FDGPU_EINVAL, "index remove: n_keep differs from the index's number of structures");
    std::vector<uint8_t> k01(n_keep);
    uint64_t S2 = 0;
    for (uint64_t s = 0; s < n_keep; ++s) { k01[s] = keep[s] ? 1u : 0u; S2 += k01[s]; }
    if (!S2) FAIL(c, FDGPU_EINVAL, "index remove: nothing kept");
    reset_timings(c);
    hipStream_t st = c->stream;
    const uint64_t H = ix->n_hashes, S = n_keep;
    if (int rc = fd_index_last_ids_staged(c, ix, "prune_last_ids")) return rc;
    const uint64_t Hx = std::max<uint64_t>(H, 1);
    HIPCHK(c, c->ws[WS_KEYS_B].ensure((S + 2) * 8 + S + 16));       // K[S + 1] (u64), then keep[S]
    HIPCHK(c, c->ws[WS_MISC0].ensure(Hx * 4));                      // sizes
    HIPCHK(c, c->ws[WS_MISC1].ensure(Hx * 4));                      // new last ids
    HIPCHK(c, c->ws[WS_MISC2].ensure(Hx * 3 + 16));                 // mode, recode flag, long flag
    HIPCHK(c, c->ws[WS_IDS_A].ensure((Hx + 1) * 8));                // recode prefix, then slots
    HIPCHK(c, c->ws[WS_IDS_B].ensure((Hx + 1) * 8));                // long prefix, then value offsets of all lists
    HIPCHK(c, c->ws[WS_KEYS_A].ensure(Hx * 4));                     // order of the re-encoded lists
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(std::max<uint64_t>(S, Hx)) * 8 + 64));
    HIPCHK(c, c->ws[WS_TOTAL].ensure(64));
    uint64_t *K = c->ws[WS_KEYS_B].as<uint64_t>();
    uint8_t *kd = (uint8_t *)(K + S + 2);
    uint32_t *sizes = c->ws[WS_MISC0].as<uint32_t>(), *nlast = c->ws[WS_MISC1].as<uint32_t>();
    uint8_t *mode = c->ws[WS_MISC2].as<uint8_t>(), *recode = mode + Hx, *is_long = mode + 2 * Hx;
    uint64_t *pre_a = c->ws[WS_IDS_A].as<uint64_t>(), *pre_b = c->ws[WS_IDS_B].as<uint64_t>();
    uint32_t *order = c->ws[WS_KEYS_A].as<uint32_t>();
    uint64_t *scan_tmp = c->ws[WS_SCANTMP].as<uint64_t>(), *tot = c->ws[WS_TOTAL].as<uint64_t>();
    // WS_TOTAL: [0] scan total, [1] removed postings, [2] error bits
    uint32_t *err = (uint32_t *)(tot + 2);
    pr_args A{ix->offsets, ix->value, ix->last_ids, H, K, S, (uint32_t)ix->first_id};
    uint64_t n_recode = 0;
    {
        StageTimer t(c, "prune_plan", S * 9 + H * 31);
        HIPCHK(c, hipMemcpyAsync(kd, k01.data(), S, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(tot + 1, 0, 16, st));
        fd_exclusive_scan<uint8_t>(kd, S, K, scan_tmp, tot, st);
        if (H) {
            hipLaunchKernelGGL(k_pr_plan, dim3(fd_grid(H, 256)), dim3(256), 0, st, A, sizes, nlast, mode, recode, is_long, err);
            fd_order_long_first(recode, is_long, H, pre_a, pre_b, scan_tmp, tot, order, nullptr, st);
        }
    }
    HIPCHK(c, hipGetLastError());
    if (H) {
        HIPCHK(c, hipMemcpyAsync(&n_recode, pre_a + H, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    uint64_t Hn = 0, Vn = 0;
    {
        StageTimer t(c, "prune_sizes", ix->value_len + H * 16);
        if (n_recode)
            hipLaunchKernelGGL((k_pr_recode<false>), dim3(fd_grid(n_recode, 4)), dim3(256), 0, st, A, order, n_recode, sizes, nlast,
                               (unsigned long long *)(tot + 1), (const uint64_t *)nullptr, (uint8_t *)nullptr, err);
        if (H) {
            hipLaunchKernelGGL(k_pr_nonzero, dim3(fd_grid(H, 256)), dim3(256), 0, st, sizes, H, recode);
            fd_exclusive_scan<uint8_t>(recode, H, pre_a, scan_tmp, tot, st);          // slots of the non-empty lists
            fd_exclusive_scan<uint32_t>(sizes, H, pre_b, scan_tmp, tot, st);          // value offsets (empty lists: 0 bytes)
        }
    }
    HIPCHK(c, hipGetLastError());
    uint64_t hv[3] = {0, 0, 0};
    uint32_t eb = 0;
    if (H) {
        HIPCHK(c, hipMemcpyAsync(&hv[0], pre_a + H, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&hv[1], pre_b + H, 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipMemcpyAsync(&hv[2], tot + 1, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&eb, err, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (eb & FD_IXERR_LONG) FAIL(c, FDGPU_ERANGE, "index remove: a posting list reaches 4 GiB");
    if (eb & FD_IXERR_DAMAGED) FAIL(c, FDGPU_EINVAL, "index remove: the index holds ids outside [first_id, first_id + n_structures)");
    Hn = hv[0]; Vn = hv[1];
    fdgpu_index *r = nullptr;
    if (int rc = fd_index_new(c, true, Hn, Vn, true, &r)) return rc;
    r->n_postings = ix->n_postings - hv[2]; r->n_structures = S2; r->first_id = ix->first_id;
    {
        StageTimer t(c, "prune_write", ix->value_len + Vn + H * 8);
        if (H) {
            if (n_recode)
                hipLaunchKernelGGL((k_pr_recode<true>), dim3(fd_grid(n_recode, 4)), dim3(256), 0, st, A, order, n_recode, sizes, nlast,
                                   (unsigned long long *)(tot + 1), pre_b, r->value, err);
            hipLaunchKernelGGL(k_pr_copy, dim3(fd_grid(H, 32)), dim3(256), 0, st, A, mode, sizes, pre_b, r->value);
            hipLaunchKernelGGL(k_pr_compact, dim3(fd_grid(H, 256)), dim3(256), 0, st, ix->hashes, sizes, nlast, pre_a, pre_b, H, r->hashes, r->offsets, r->last_ids);
        } else {
            (void)hipMemsetAsync(r->offsets, 0, 8, st);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("index remove write: ") + hipGetErrorString(e); return fd_index_op_failed(c, FDGPU_EHIP, &r); }
    *out = r;
    return FDGPU_OK;
}
