// k_rows.hip — rows of the transposed index (fdgpu_index_rows): for the structures id_lo .. id_hi - 1 of a resident index, the ascending hashes
// whose posting lists hold each of them.  The output has the shape of fdgpu_hash_batch(sort_dedup = 1), and equals it for the same structures.
//
// It is the build's sort run the other way.  The build sorts an id-major key stream stably by hash; a resident index is a hash-major stream of
// (hash, id), and a stable sort of it by id leaves, per structure, its hashes ascending.  Only the postings of the window enter the stream:
//
//   k_rw_plan      thread per list: offsets checked, the list's last byte must end a varint, the head (first varint) must be an id of the index.
//                  A list is ascending, so it is SELECTED only if its head is below id_hi and (where the index carries last ids) its last id is
//                  not below id_lo; the others hold nothing of the window and are not walked.  cnt[t] = 0
//   order          the selected lists in the order the walks take them, lists of FD_LONG_LIST_BYTES and more first (fd_order_long_first)
//   k_rw_walk<0>   wavefront per selected list (fd_wave_walk, 256 bytes per step): every varint's form and every id (fd_id_local) checked,
//                  cnt[t] = the list's ids inside [id_lo, id_hi).  The call fails behind this kernel if anything was damaged: nothing is emitted
//   scan           the shared exclusive scan over cnt in LIST order: base[t] = the list's place in the stream, base[H] = its length n
//   k_rw_walk<1>   the same walk, the same predicate: the k-th id of list t inside the window goes to key[base[t] + k] = id - id_lo,
//                  val[base[t] + k] = hashes[t]; a step's ids of the window leave as one contiguous run (start bits, a wave scan, a store per
//                  start).  The stream is ordered by (hash, id), deterministic, and needed no atomic
//   sort           fd_radix_sort_pairs by the bits of id_hi - id_lo - 1 in the build's sort workspaces: stable, so a row's hashes stay ascending.
//                  A window of one structure has no key bit: the stream already is its row, and the sort is not called
//   k_rw_bounds    thread per row boundary s = 0 .. W: row_off[s] = the number of sorted keys below s, by a binary search of the sorted keys.
//                  Empty rows come out right without a histogram and without atomics, and no thread's work depends on the width of a gap
//                  between two keys (a thread per sorted element would fill such a gap alone: 2^24 stores for one sparse window)
// Everything up to the bounds is one stage, fd_rows_device, that leaves val, row_off and n in the context's workspaces; the rows copy them out
// behind it, the signatures (k_sig.hip) reduce them where they are.
// Byte work: the value bytes of the selected lists are read twice (count, emit); the emit writes 8 bytes per window posting; the sort reads and
// writes 16 bytes per window posting in each of ceil(key_bits / 8) passes; the bounds gather ceil(log2(n + 1)) keys per row and write 8 bytes.
// Workspace: 16 bytes per window posting, 34 bytes per list, 8 bytes per window structure — see DESIGN.md §4f.
#include <cstring>
#include "fdgpu_internal.h"
#include "fd_api_common.h"
#include "fd_postings.h"

struct rw_args {
    const uint32_t *hashes; const uint64_t *offsets; const uint8_t *value; const uint32_t *last_ids;
    uint64_t H, value_len, S; uint32_t first_id; uint64_t id_lo, id_hi;
};

// ---- plan: thread per list.  Reads the 8 bytes at value + b0 only for b0 < b1 <= value_len (FD_VALUE_SLACK)
__global__ __launch_bounds__(256) void k_rw_plan(rw_args A, uint8_t *__restrict__ sel, uint8_t *__restrict__ is_long, uint32_t *__restrict__ cnt,
                                                 uint32_t *__restrict__ err) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.H) return;
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    uint32_t bad = 0, s = 0;
    if (b1 <= b0 || b1 > A.value_len) bad = FD_IXERR_DAMAGED;
    else if (b1 - b0 > 0xffffffffull) bad = FD_IXERR_LONG;
    else {
        uint32_t nf = 0;
        const uint32_t head = fd_first_varint(A.value + b0, &nf);
        uint64_t loc;
        if (nf == 0 || nf > b1 - b0 || (A.value[b1 - 1] & 0x80u) || !fd_id_local(head, A.first_id, A.S, &loc)) bad = FD_IXERR_DAMAGED;
        else s = head < A.id_hi && (!A.last_ids || A.last_ids[t] >= A.id_lo) ? 1u : 0u;
    }
    if (bad) atomicOr(err, bad);
    sel[t] = (uint8_t)s;
    is_long[t] = (uint8_t)(s && b1 - b0 >= FD_LONG_LIST_BYTES ? 1u : 0u);
    cnt[t] = 0u;
}

// ---- the walk: wavefront per selected list; launched only behind a plan that found every offset sound.  W = false: checks and cnt[t];
// W = true: the stream.  Both passes test an id with the same expression, so base[t] + k stays below base[t + 1] whatever the bytes hold.
template <bool W>
__global__ __launch_bounds__(256) void k_rw_walk(rw_args A, const uint32_t *__restrict__ order, uint64_t n_lists, uint32_t *__restrict__ cnt,
                                                 const uint64_t *__restrict__ base, uint32_t *__restrict__ key, uint32_t *__restrict__ val,
                                                 uint32_t *__restrict__ err) {
    const uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= n_lists) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = order[g];
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    const uint64_t at = W ? base[t] : 0;
    const uint32_t h = W ? A.hashes[t] : 0u;
    uint32_t run = 0;             // ids of the window so far
    bool bad = false;
    fd_wave_walk(A.value, b0, b1, lane, [&](const fd_step &ds, uint32_t id0) {
        uint32_t in = 0;          // the lane's starts whose id lies in the window
        fd_lane_starts(ds, id0, [&](uint32_t j, uint32_t id) {
            uint64_t loc;
            // no end in five bytes, or a fifth byte with more than four value bits; an id that is not the index's
            if (ds.nf[j] == 0 || (ds.nf[j] == 5 && ((uint32_t)(ds.win >> (8u * j + 32u)) & 0x70u)) || !fd_id_local(id, A.first_id, A.S, &loc)) bad = true;
            if (id >= A.id_lo && id < A.id_hi) in |= 1u << j;
        });
        const uint32_t n_in = (uint32_t)__popc(in), inc = fd_wave_scan_add(n_in, lane);
        if (W) {
            uint64_t o = at + run + (inc - n_in);
            fd_lane_starts(ds, id0, [&](uint32_t j, uint32_t id) {
                if ((in >> j) & 1u) { key[o] = (uint32_t)(id - A.id_lo); val[o] = h; ++o; }
            });
        }
        run += __shfl(inc, FD_WAVE - 1, FD_WAVE);
    });
    if (!W) {
        if (bad) atomicOr(err, FD_IXERR_DAMAGED);
        if (lane == 0) cnt[t] = run;      // a list of less than 4 GiB holds fewer than 2^32 ids
    }
}

// ---- bounds: row_off[s] = sorted keys below s (s = W: all n of them)
__global__ __launch_bounds__(256) void k_rw_bounds(const uint32_t *__restrict__ key, uint64_t n, uint64_t W, uint64_t *__restrict__ row_off) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > W) return;
    uint64_t lo = 0, hi = n;      // keys below lo are < s, keys from hi on are >= s
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < s) lo = mid + 1; else hi = mid;
    }
    row_off[s] = lo;
}

// ---- the device stage: plan -> count -> scan -> emit -> sort -> bounds.  Leaves the window's rows in the context's workspaces: out->val (the n
// hashes in (id, hash) order), out->row_off (W + 1 offsets) — valid until the context's next call that uses its sort workspaces.  `what` opens
// the messages ("index rows", "index signatures").  The stream is not synchronised behind the last kernel.
int fd_rows_device(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t id_lo, uint64_t id_hi, const char *what, fd_rows_dev *out) {
    hipStream_t st = c->stream;
    const uint64_t H = ix->n_hashes, W = id_hi - id_lo;
    const std::string pre = std::string(what) + ": ";
    uint64_t n = 0;               // postings inside the window
    uint32_t *val = nullptr;      // their hashes in (id, hash) order, on the device
    HIPCHK(c, c->ws[WS_MISC5].ensure((W + 1) * 8));
    uint64_t *row_off = c->ws[WS_MISC5].as<uint64_t>();
    if (H && W) {
        HIPCHK(c, c->ws[WS_MISC0].ensure(H * 4));                       // order of the selected lists
        HIPCHK(c, c->ws[WS_MISC1].ensure(H * 4));                       // cnt
        HIPCHK(c, c->ws[WS_MISC2].ensure(H * 2));                       // selected, long
        HIPCHK(c, c->ws[WS_MISC3].ensure((H + 1) * 8));                 // selected lists before each list
        HIPCHK(c, c->ws[WS_MISC4].ensure((H + 1) * 8));                 // long ones before each list
        HIPCHK(c, c->ws[WS_SEGOFF].ensure((H + 1) * 8));                // base
        HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(H) * 8 + 64));
        HIPCHK(c, c->ws[WS_TOTAL].ensure(64));                          // [0] scan total, [1] error bits
        uint32_t *order = c->ws[WS_MISC0].as<uint32_t>(), *cnt = c->ws[WS_MISC1].as<uint32_t>();
        uint8_t *sel = c->ws[WS_MISC2].as<uint8_t>(), *is_long = sel + H;
        uint64_t *sel_pre = c->ws[WS_MISC3].as<uint64_t>(), *long_pre = c->ws[WS_MISC4].as<uint64_t>(), *base = c->ws[WS_SEGOFF].as<uint64_t>();
        uint64_t *scan_tmp = c->ws[WS_SCANTMP].as<uint64_t>(), *tot = c->ws[WS_TOTAL].as<uint64_t>();
        uint32_t *err = (uint32_t *)(tot + 1);
        const rw_args A{ix->hashes, ix->offsets, ix->value, ix->last_ids, H, ix->value_len, ix->n_structures, (uint32_t)ix->first_id, id_lo, id_hi};
        {
            StageTimer t(c, "rows_plan", H * (16 + 8 + 1 + (ix->last_ids ? 4 : 0) + 6 + 2 * (1 + 8) + 4));
            HIPCHK(c, hipMemsetAsync(tot, 0, 16, st));
            hipLaunchKernelGGL(k_rw_plan, dim3(fd_grid(H, 256)), dim3(256), 0, st, A, sel, is_long, cnt, err);
            fd_order_long_first(sel, is_long, H, sel_pre, long_pre, scan_tmp, tot, order, nullptr, st);
        }
        HIPCHK(c, hipGetLastError());
        uint64_t n_sel = 0, hv[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(&n_sel, sel_pre + H, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(&hv[1], tot + 1, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (hv[1] & FD_IXERR_DAMAGED)
            FAIL(c, FDGPU_EINVAL, pre + "the index is damaged (offsets that do not ascend inside the value bytes, or a list whose first id is outside "
                                        "[first_id, first_id + n_structures))");
        if (hv[1] & FD_IXERR_LONG) FAIL(c, FDGPU_ERANGE, pre + "a posting list reaches 4 GiB");
        if (n_sel) {
            StageTimer t(c, "rows_count", ix->value_len + n_sel * (4 + 16 + 4));      // at most: the selected lists' bytes
            hipLaunchKernelGGL((k_rw_walk<false>), dim3(fd_grid(n_sel, 4)), dim3(256), 0, st, A, order, n_sel, cnt, (const uint64_t *)nullptr,
                               (uint32_t *)nullptr, (uint32_t *)nullptr, err);
        }
        {
            StageTimer t(c, "rows_scan", H * (4 + 8));
            fd_exclusive_scan<uint32_t>(cnt, H, base, scan_tmp, tot, st);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hv, tot, sizeof hv, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (hv[1] & FD_IXERR_DAMAGED)
            FAIL(c, FDGPU_EINVAL, pre + "the index is damaged (a varint that leaves its list, or ids outside [first_id, first_id + n_structures))");
        if (hv[0] > 0xffffffffull) FAIL(c, FDGPU_ERANGE, pre + "2^32 or more postings inside the window; take a narrower window");
        n = hv[0];
        if (n) {
            const size_t kb = n * 4;
            if (kb > c->ws[WS_KEYS_A].cap + ((size_t)1 << 30)) c->pool_drop();      // gigabytes of sort buffers: the cached blocks of destroyed indices go back first
            HIPCHK(c, c->ws[WS_KEYS_A].ensure(kb));
            HIPCHK(c, c->ws[WS_IDS_A].ensure(kb + 16));                             // the sizes of the build's sort buffers (ensure_sort_ws)
            uint32_t *ka = c->ws[WS_KEYS_A].as<uint32_t>(), *va = c->ws[WS_IDS_A].as<uint32_t>();
            int key_bits = 0;
            while (key_bits < 32 && (1ull << key_bits) < W) ++key_bits;             // bits of W - 1
            if (key_bits) {
                HIPCHK(c, c->ws[WS_KEYS_B].ensure(kb));
                HIPCHK(c, c->ws[WS_IDS_B].ensure(kb + 16));
                HIPCHK(c, c->ws[WS_GHIST].ensure((size_t)256 * std::max<uint32_t>(fd_rs_num_tiles(n), 1) * 4));
                HIPCHK(c, c->ws[WS_TOT].ensure((256 + (size_t)(fd_rs_num_tiles(n) / 128 + 2) * 256) * 8));
            }
            {
                StageTimer t(c, "rows_emit", ix->value_len + n * 8 + n_sel * (4 + 16 + 8 + 4));
                hipLaunchKernelGGL((k_rw_walk<true>), dim3(fd_grid(n_sel, 4)), dim3(256), 0, st, A, order, n_sel, cnt, base, ka, va, err);
            }
            val = va;
            if (key_bits) {       // no key bit: one structure, the stream is its row
                uint32_t *kb2 = c->ws[WS_KEYS_B].as<uint32_t>(), *vb = c->ws[WS_IDS_B].as<uint32_t>();
                const int cur = sort_pairs(c, ka, va, kb2, vb, n, key_bits);
                if (cur) { ka = kb2; val = vb; }
            }
            {
                StageTimer t(c, "rows_bounds", (W + 1) * 8);
                hipLaunchKernelGGL(k_rw_bounds, dim3(fd_grid(W + 1, 256)), dim3(256), 0, st, ka, n, W, row_off);
            }
            HIPCHK(c, hipGetLastError());
        }
    }
    if (!n) HIPCHK(c, hipMemsetAsync(row_off, 0, (W + 1) * 8, st));      // no posting in the window: every row is empty
    out->val = val; out->row_off = row_off; out->n = n;
    return FDGPU_OK;
}

// ---- rows = the device stage, then the copy out
static int rows_impl(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t id_lo, uint64_t id_hi, uint32_t **out_h, uint64_t **out_off) {
    reset_timings(c);
    hipStream_t st = c->stream;
    const uint64_t W = id_hi - id_lo;
    fd_rows_dev R;
    const int rc = fd_rows_device(c, ix, id_lo, id_hi, "index rows", &R);
    if (rc != FDGPU_OK) return rc;
    const uint64_t n = R.n;
    const uint32_t *val = R.val;
    const uint64_t *row_off = R.row_off;
    uint32_t *h = (uint32_t *)fd_out_alloc(std::max<uint64_t>(n, 1) * 4);
    uint64_t *ro = (uint64_t *)fd_out_alloc((W + 1) * 8);
    if (!h || !ro) { fdgpu_free(h); fdgpu_free(ro); FAIL(c, FDGPU_ENOMEM, "index rows: out of host memory"); }
    hipError_t e = hipSuccess;
    {
        StageTimer t(c, "rows_copy", n * 4 + (W + 1) * 8);
        if (n) {
            e = fd_d2h_big(c, h, val, n * 4);             // gigabytes for a wide window: through the pinned slots, like an export
            if (e == hipSuccess) e = fd_d2h_big(c, ro, row_off, (W + 1) * 8);
        } else memset(ro, 0, (W + 1) * 8);      // no posting in the window: every row is empty
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // the result is complete, and the context's workspaces free again, when the call returns
    if (e != hipSuccess) { fdgpu_free(h); fdgpu_free(ro); c->err = std::string("index rows: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    *out_h = h; *out_off = ro;
    return FDGPU_OK;
}

extern "C" int fdgpu_index_rows(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t id_lo, uint64_t id_hi, uint32_t **hashes, uint64_t **row_off) { FD_LOCK(c);
    if (!c || !ix || !hashes || !row_off) return FDGPU_EINVAL;
    *hashes = nullptr; *row_off = nullptr;
    if (id_lo < ix->first_id || id_lo > id_hi || id_hi > ix->first_id + ix->n_structures)
        FAIL(c, FDGPU_EINVAL, "index rows: the window is not inside [first_id, first_id + n_structures]");
    const int rc = rows_impl(c, ix, id_lo, id_hi, hashes, row_off);
    if (rc != FDGPU_OK) (void)hipStreamSynchronize(c->stream);      // nothing of a failed call is still running when it returns
    return rc;
}
