// k_permute.hip — device-side reorder of the structures of a resident index (fdgpu_index_permute): the structure at local position k moves to
// position new_id[k]; the result equals, byte for byte, a build over the same structures taken in the new order.
//
// Every other index operation keeps a list's ids ascending and re-deltas it in one walk.  Under a permutation the mapped ids of a list come out in
// any order and have to be put back in ascending order before they can be delta-encoded: a sort per list.  Lists are independent, so each is
// ordered on its own, in LDS or in a bitmap; nothing is sized by the total number of postings.  A list of b bytes holds at most b ids (a varint
// has at least one byte), so the byte length — known from the offsets alone — bounds what a list needs:
//
//   SORT    lists of at most PM_SORT_BYTES bytes (the bulk): one wavefront per list.  The mapped ids go to the wavefront's LDS buffer while the list
//           is decoded (fd_wave_walk, 256 bytes per step); ids that are already ascending are left alone (the identity, or a permutation that
//           keeps the order of this list's ids), the others take a bitonic network on the next power of two, then 64 ids per step are re-delta'd
//   BITMAP  longer lists: one workgroup per list and a bitmap of n_structures bits — a posting list is a set of ids in [0, n), so setting bit
//           new_id[id] for every decoded id and reading the bitmap in ascending order sorts it without a comparison.  The workgroup decodes
//           2 KiB per step (eight wavefronts, one fd_decode_step and fd_lane_starts each, their id sums joined through LDS), then takes 512 bitmap words per step:
//           popcount gives a word's ids, a workgroup scan of the varint lengths their places, a workgroup max scan the id in front of a word.
//           The bitmap lives in the workgroup's LDS while n_structures <= PM_LDS_BITS (160 KiB less the scan scratch: 1,308,672 bits), beyond that
//           in a global-memory slab of ceil(n / 32) words per workgroup, cleared per list, with a bounded number of slabs.
//
//   k_pm_plan     thread per list: offsets checked, class by byte length, bytes of the BITMAP class
//   order         lists in the order the kernels take them: BITMAP lists first, each class in list order (fd_order_long_first over every list,
//                 shared with k_prune.hip and k_split.hip)
//   k_pm_sort<W>  wavefront per SORT list; W = 0: new byte size and last id, W = 1: the bytes
//   k_pm_bitmap<W, SLAB>  workgroup per BITMAP list (grid-stride over them); SLAB = 0: LDS bitmap, 1: global slab
// Both passes run the same code up to the store, so they cannot disagree about a size.  The BITMAP kernels are launched before the SORT kernel in
// either pass.  Value bytes are read twice and written once, 16 bytes of tables per hash, and new_id is gathered once per posting and pass.
// Workspace: 17 bytes per list, 4 bytes per structure, the slabs (at most PM_SLAB_BYTES in all) — see DESIGN.md §4d.
#include "fdgpu_internal.h"
#include "fd_api_common.h"
#include "fd_postings.h"

#define PM_SORT_BYTES 2048u                                   // SORT class: lists up to this many bytes, hence ids (8 KiB of LDS per wavefront)
#define PM_SORT_WAVES 4u                                      // lists per workgroup of k_pm_sort (32 KiB of LDS: five workgroups, 20 wavefronts per CU)
#define PM_BM_THREADS 512u                                    // k_pm_bitmap: eight wavefronts per list
#define PM_BM_WAVES (PM_BM_THREADS / FD_WAVE)
#define PM_BM_SCRATCH 64u                                     // words of k_pm_bitmap's LDS in front of the bitmap (scan partials)
#define PM_LDS_BITS ((160u * 1024u - PM_BM_SCRATCH * 4u) * 8u)      // ids a workgroup's LDS bitmap covers
#define PM_SLAB_BYTES (1ull << 30)                            // all global bitmap slabs together

struct pm_args { const uint64_t *offsets; const uint8_t *value; uint64_t H, value_len, S; const uint32_t *new_id; uint32_t first_id; };

// ---- plan: thread per list.  A list with bad offsets is flagged and put into the SORT class; the call fails behind this kernel, nothing decodes it
__global__ __launch_bounds__(256) void k_pm_plan(pm_args A, uint32_t sort_bytes, uint8_t *__restrict__ is_long, unsigned long long *__restrict__ long_bytes,
                                                 uint32_t *__restrict__ err) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.H) return;
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    uint32_t lg = 0;
    if (b1 <= b0 || b1 > A.value_len) atomicOr(err, FD_IXERR_DAMAGED);
    else if (b1 - b0 > 0xffffffffull) atomicOr(err, FD_IXERR_LONG);
    else if (b1 - b0 > sort_bytes) { lg = 1; atomicAdd(long_bytes, (unsigned long long)(b1 - b0)); }
    is_long[t] = (uint8_t)lg;
}

// ---- SORT class: wavefront per list.  buf holds at most PM_SORT_BYTES ids: every id starts at a byte of its own inside a list of at most that many
template <bool W>
__global__ __launch_bounds__(PM_SORT_WAVES * FD_WAVE) void k_pm_sort(pm_args A, const uint32_t *__restrict__ order, uint64_t n_lists, uint32_t *__restrict__ sizes,
                                                                uint32_t *__restrict__ new_last, const uint64_t *__restrict__ out_off,
                                                                uint8_t *__restrict__ out_value, uint32_t *__restrict__ err) {
    __shared__ uint32_t lds[PM_SORT_WAVES][PM_SORT_BYTES];
    const uint64_t g = (uint64_t)blockIdx.x * PM_SORT_WAVES + (threadIdx.x >> 6);
    if (g >= n_lists) return;                     // whole wavefronts leave: no workgroup barrier in this kernel
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t *buf = lds[threadIdx.x >> 6];
    const uint64_t t = order[g];
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    // decode and map
    uint32_t cnt = 0;
    bool bad = false;
    fd_wave_walk(A.value, b0, b1, lane, [&](const fd_step &ds, uint32_t id0) {
        const uint32_t ns = (uint32_t)__popc(ds.sb), sinc = fd_wave_scan_add(ns, lane);
        uint32_t pos = cnt + sinc - ns;
        fd_lane_starts(ds, id0, [&](uint32_t, uint32_t id) {
            uint64_t loc;
            uint32_t m = A.first_id;
            if (!fd_id_local(id, A.first_id, A.S, &loc)) bad = true;
            else m = A.first_id + A.new_id[loc];
            if (pos < PM_SORT_BYTES) buf[pos] = m;
            ++pos;
        });
        cnt += __shfl(sinc, FD_WAVE - 1, FD_WAVE);
    });
    if (cnt > PM_SORT_BYTES) cnt = PM_SORT_BYTES;      // cannot happen (see above); keeps every LDS index in range whatever the bytes are
    if (bad) atomicOr(err, FD_IXERR_DAMAGED);
    fd_wave_lds_fence();
    // already ascending?
    bool desc = false;
    for (uint32_t i = lane; i + 1 < cnt; i += 64) desc |= buf[i] > buf[i + 1];
    if (__any(desc)) {
        uint32_t m = 2;
        while (m < cnt) m <<= 1;
        for (uint32_t i = cnt + lane; i < m; i += 64) buf[i] = 0xffffffffu;      // above every id: first_id + n_structures <= 2^32 - 1
        fd_wave_lds_fence();
        for (uint32_t k = 2; k <= m; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = lane; i < (m >> 1); i += 64) {
                    const uint32_t lo = ((i & ~(j - 1u)) << 1) | (i & (j - 1u)), hi = lo | j;
                    const uint32_t a = buf[lo], b = buf[hi];
                    if ((a > b) == ((lo & k) == 0u)) { buf[lo] = b; buf[hi] = a; }
                }
                fd_wave_lds_fence();
            }
        }
    }
    // re-delta, 64 ids per step
    uint8_t *dst = W ? out_value + out_off[t] : nullptr;
    uint32_t out_pos = 0;
    for (uint32_t c0 = 0; c0 < cnt; c0 += 64) {
        const uint32_t i = c0 + lane;
        uint32_t d = 0, ln = 0;
        if (i < cnt) {
            d = i ? buf[i] - buf[i - 1] : buf[0];
            ln = fd_varint_len(d);
        }
        const uint32_t linc = fd_wave_scan_add(ln, lane);
        if (W) fd_varint_store(dst + out_pos + (linc - ln), d, ln);
        out_pos += __shfl(linc, FD_WAVE - 1, FD_WAVE);
    }
    if (!W && lane == 0) {
        sizes[t] = out_pos;                           // at most 5 * PM_SORT_BYTES
        new_last[t] = cnt ? buf[cnt - 1] : 0u;
    }
}

// ---- BITMAP class: workgroup per list, grid-stride over the lists.  Dynamic LDS: PM_BM_SCRATCH words, then (SLAB = false) the bitmap.
// Bits are set only at new_id values, which the host has checked to lie below S, so every bitmap index is below ceil(S / 32).
template <bool W, bool SLAB>
__global__ __launch_bounds__(PM_BM_THREADS) void k_pm_bitmap(pm_args A, const uint32_t *__restrict__ order, uint64_t n_lists, uint32_t *slabs,
                                                             uint32_t *__restrict__ sizes, uint32_t *__restrict__ new_last,
                                                             const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out_value,
                                                             uint32_t *__restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pm_lds[];
    uint32_t *s_id = pm_lds, *s_max = pm_lds + 16, *s_len = pm_lds + 24;      // [2][8] id sums of a decode step, [8] last set bits, [8] varint bytes
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t words = (uint32_t)((A.S + 31u) >> 5);
    uint32_t *bm = SLAB ? slabs + (uint64_t)blockIdx.x * words : pm_lds + PM_BM_SCRATCH;
    for (uint64_t g = blockIdx.x; g < n_lists; g += gridDim.x) {
        const uint64_t t = order[g];
        const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
        for (uint32_t w = tid; w < words; w += PM_BM_THREADS) bm[w] = 0u;
        __syncthreads();
        // decode and map: eight steps of 256 bytes at a time, one per wavefront
        uint32_t run_id = 0, it = 0;
        bool bad = false;
        for (uint64_t base = b0; base < b1; base += 256u * PM_BM_WAVES, it ^= 1u) {
            const uint64_t wb = base + 256u * wave, p = wb + 4u * lane, pn = p + 256;
            const uint32_t cur = p < b1 ? fd_load4(A.value + p) : 0u, nxt = pn < b1 ? fd_load4(A.value + pn) : 0u;
            const bool term_before = wb == b0 || wb >= b1 || !(A.value[wb - 1] & 0x80u);      // this wavefront's step starts a varint: from the byte before it
            fd_step ds;
            fd_decode_step(cur, nxt, p, b1, lane, term_before, &ds);
            const uint32_t dinc = fd_wave_scan_add(ds.dsum, lane);
            if (lane == FD_WAVE - 1) s_id[it * 8u + wave] = dinc;
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (uint32_t k = 0; k < PM_BM_WAVES; ++k) { const uint32_t v = s_id[it * 8u + k]; before += k < wave ? v : 0u; total += v; }
            fd_lane_starts(ds, run_id + before + dinc - ds.dsum, [&](uint32_t, uint32_t id) {
                uint64_t loc;
                if (!fd_id_local(id, A.first_id, A.S, &loc)) bad = true;
                else { const uint32_t q = A.new_id[loc]; atomicOr(&bm[q >> 5], 1u << (q & 31u)); }
            });
            run_id += total;      // s_id[it] is written again two steps on, behind the next step's barrier
        }
        if (bad) atomicOr(err, FD_IXERR_DAMAGED);
        __syncthreads();
        // the bitmap in ascending order, 512 words per step
        uint8_t *dst = W ? out_value + out_off[t] : nullptr;
        uint32_t prev1 = 0;           // local position + 1 of the last id so far, 0 = none yet
        uint64_t out_pos = 0;
        for (uint32_t w0 = 0; w0 < words; w0 += PM_BM_THREADS) {
            const uint32_t w = w0 + tid;
            uint32_t word = 0;
            if (w < words) word = SLAB ? __hip_atomic_load(&bm[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : bm[w];
            const uint32_t mylast = word ? (w << 5) + (32u - (uint32_t)__clz(word)) : 0u;
            const uint32_t lmax = fd_wave_scan_max(mylast, lane);
            if (lane == FD_WAVE - 1) s_max[wave] = lmax;
            __syncthreads();
            uint32_t pred = __shfl_up(lmax, 1, FD_WAVE), tile_max = prev1;
            if (lane == 0) pred = 0;
            if (prev1 > pred) pred = prev1;
#pragma unroll
            for (uint32_t k = 0; k < PM_BM_WAVES; ++k) {
                const uint32_t v = s_max[k];
                if (k < wave && v > pred) pred = v;
                if (v > tile_max) tile_max = v;
            }
            uint32_t lsum = 0, q1 = pred;
            for (uint32_t r = word; r; r &= r - 1u) {
                const uint32_t pos = (w << 5) + (uint32_t)__ffs(r) - 1u;
                lsum += fd_varint_len(q1 ? pos + 1u - q1 : A.first_id + pos);
                q1 = pos + 1u;
            }
            const uint32_t linc = fd_wave_scan_add(lsum, lane);
            if (lane == FD_WAVE - 1) s_len[wave] = linc;
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (uint32_t k = 0; k < PM_BM_WAVES; ++k) { const uint32_t v = s_len[k]; before += k < wave ? v : 0u; total += v; }
            if (W) {
                uint8_t *o = dst + out_pos + before + (linc - lsum);
                q1 = pred;
                for (uint32_t r = word; r; r &= r - 1u) {
                    const uint32_t pos = (w << 5) + (uint32_t)__ffs(r) - 1u;
                    const uint32_t d = q1 ? pos + 1u - q1 : A.first_id + pos, ln = fd_varint_len(d);
                    fd_varint_store(o, d, ln);
                    o += ln;
                    q1 = pos + 1u;
                }
            }
            out_pos += total;
            prev1 = tile_max;      // s_max is written again behind the next step's first barrier, s_len behind its second
        }
        if (!W && tid == 0) {
            if (out_pos > 0xffffffffull) { atomicOr(err, FD_IXERR_LONG); out_pos = 0; }
            sizes[t] = (uint32_t)out_pos;
            new_last[t] = prev1 ? A.first_id + (prev1 - 1u) : 0u;
        }
        __syncthreads();          // every read of the bitmap is behind us before the next list clears it
    }
}

static uint32_t pm_switch(const char *name, uint32_t dflt) {      // test switches: they only lower a boundary
    const char *e = getenv(name);
    const long long v = e ? atoll(e) : 0;
    return v > 0 && (unsigned long long)v < dflt ? (uint32_t)v : dflt;
}

template <bool W>
static hipError_t pm_launch_bitmap(bool slab, unsigned grid, size_t lds, hipStream_t st, const pm_args &A, const uint32_t *order, uint64_t n_long,
                                   uint32_t *slabs, uint32_t *sizes, uint32_t *nlast, const uint64_t *out_off, uint8_t *out_value, uint32_t *err) {
    if (slab) {
        hipLaunchKernelGGL((k_pm_bitmap<W, true>), dim3(grid), dim3(PM_BM_THREADS), lds, st, A, order, n_long, slabs, sizes, nlast, out_off, out_value, err);
        return hipSuccess;
    }
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pm_bitmap<W, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_pm_bitmap<W, false>), dim3(grid), dim3(PM_BM_THREADS), lds, st, A, order, n_long, slabs, sizes, nlast, out_off, out_value, err);
    return hipSuccess;
}

static int permute_impl(fdgpu_ctx *c, const fdgpu_index *ix, const uint32_t *new_id, fdgpu_index **out) {
    reset_timings(c);
    hipStream_t st = c->stream;
    const uint64_t H = ix->n_hashes, S = ix->n_structures;
    fdgpu_index *nx = nullptr;
    if (int rc = fd_index_new(c, true, H, H ? FD_VALUE_LATER : 0, H != 0, &nx)) return rc;
    *out = nx;
    nx->n_postings = ix->n_postings; nx->n_structures = S; nx->first_id = ix->first_id;
    if (!H) {
        HIPCHK(c, hipMemsetAsync(nx->offsets, 0, 8, st));
        HIPCHK(c, hipStreamSynchronize(st));
        return FDGPU_OK;
    }
    const uint32_t sort_bytes = pm_switch("FDGPU_PERM_SORT_BYTES", PM_SORT_BYTES), lds_bits = pm_switch("FDGPU_PERM_LDS_BITS", PM_LDS_BITS);
    const bool slab = S > lds_bits;
    const uint64_t words = (S + 31) >> 5;
    HIPCHK(c, c->ws[WS_MISC0].ensure(H * 4));                       // new byte length of every list
    HIPCHK(c, c->ws[WS_MISC2].ensure(H));                           // class of every list
    HIPCHK(c, c->ws[WS_IDS_A].ensure((H + 1) * 8));                 // BITMAP lists before each list
    HIPCHK(c, c->ws[WS_KEYS_A].ensure(H * 4));                      // order of the lists
    HIPCHK(c, c->ws[WS_KEYS_B].ensure(std::max<uint64_t>(S, 1) * 4));      // new_id
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(H) * 8 + 64));
    HIPCHK(c, c->ws[WS_TOTAL].ensure(64));                          // [0] scan total, [1] error bits, [2] bytes of the BITMAP class
    uint32_t *sizes = c->ws[WS_MISC0].as<uint32_t>(), *order = c->ws[WS_KEYS_A].as<uint32_t>(), *nid = c->ws[WS_KEYS_B].as<uint32_t>();
    uint8_t *is_long = c->ws[WS_MISC2].as<uint8_t>();
    uint64_t *lpre = c->ws[WS_IDS_A].as<uint64_t>(), *tot = c->ws[WS_TOTAL].as<uint64_t>();
    uint32_t *err = (uint32_t *)(tot + 1);
    pm_args A{ix->offsets, ix->value, H, ix->value_len, S, nid, (uint32_t)ix->first_id};
    {
        StageTimer t(c, "permute_plan", S * 8 + H * (16 + 1 + 1 + 8 + 1 + 8 + 4));
        HIPCHK(c, hipMemcpyAsync(nid, new_id, S * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(tot, 0, 24, st));
        hipLaunchKernelGGL(k_pm_plan, dim3(fd_grid(H, 256)), dim3(256), 0, st, A, sort_bytes, is_long, (unsigned long long *)(tot + 2), err);
        fd_order_long_first(nullptr, is_long, H, nullptr, lpre, c->ws[WS_SCANTMP].as<uint64_t>(), tot, order, nullptr, st);
    }
    HIPCHK(c, hipGetLastError());
    uint64_t hv[3] = {0, 0, 0};      // BITMAP lists, error bits, their bytes
    HIPCHK(c, hipMemcpyAsync(hv, tot, sizeof hv, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (hv[1] & FD_IXERR_DAMAGED) FAIL(c, FDGPU_EINVAL, "index permute: the index is damaged (offsets that do not ascend inside the value bytes)");
    if (hv[1] & FD_IXERR_LONG) FAIL(c, FDGPU_ERANGE, "index permute: a posting list reaches 4 GiB");
    const uint64_t n_long = hv[0], n_short = H - n_long, long_bytes = hv[2];
    // BITMAP launch shape: a grid-stride loop over the lists; as many workgroups as fit the CUs (LDS) or as there are slabs
    unsigned bm_grid = 0;
    size_t bm_lds = PM_BM_SCRATCH * 4;
    uint32_t *slabs = nullptr;
    if (n_long) {
        int cus = 0;
        HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        uint64_t g = std::min<uint64_t>(n_long, 2ull * (uint64_t)std::max(cus, 1));
        if (slab) {
            g = std::max<uint64_t>(1, std::min<uint64_t>(g, PM_SLAB_BYTES / (words * 4)));
            HIPCHK(c, c->ws[WS_IDS_B].ensure(g * words * 4));
            slabs = c->ws[WS_IDS_B].as<uint32_t>();
        } else bm_lds += words * 4;
        bm_grid = (unsigned)g;
    }
    const char *bm_sizes = slab ? "permute_sizes_slab" : "permute_sizes_lds", *bm_write = slab ? "permute_write_slab" : "permute_write_lds";
    const uint64_t bm_bits = (slab ? 3 : 0) * words * 4 * n_long;      // a slab is cleared, set and read in HBM
    if (n_long) {
        StageTimer t(c, bm_sizes, long_bytes + n_long * 24 + bm_bits);
        HIPCHK(c, pm_launch_bitmap<false>(slab, bm_grid, bm_lds, st, A, order, n_long, slabs, sizes, nx->last_ids, nullptr, nullptr, err));
    }
    if (n_short) {
        StageTimer t(c, "permute_sizes_sort", ix->value_len - long_bytes + n_short * 24);
        hipLaunchKernelGGL((k_pm_sort<false>), dim3(fd_grid(n_short, PM_SORT_WAVES)), dim3(PM_SORT_WAVES * FD_WAVE), 0, st, A, order + n_long, n_short, sizes,
                           nx->last_ids, (const uint64_t *)nullptr, (uint8_t *)nullptr, err);
    }
    {
        StageTimer t(c, "permute_scan", H * (4 + 8 + 4 + 4));
        fd_exclusive_scan<uint32_t>(sizes, H, nx->offsets, c->ws[WS_SCANTMP].as<uint64_t>(), tot, st);
        HIPCHK(c, hipMemcpyAsync(nx->hashes, ix->hashes, H * 4, hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hv, tot, 16, hipMemcpyDeviceToHost, st));      // new value length, error bits
    HIPCHK(c, hipStreamSynchronize(st));
    if (hv[1] & FD_IXERR_DAMAGED)
        FAIL(c, FDGPU_EINVAL, "index permute: the index holds ids outside [first_id, first_id + n_structures)");
    if (hv[1] & FD_IXERR_LONG) FAIL(c, FDGPU_ERANGE, "index permute: a posting list reaches 4 GiB");
    nx->value_len = hv[0];
    HIPCHK(c, fd_index_block(c, hv[0] + FD_VALUE_SLACK, (void **)&nx->value, &nx->cap_value));
    if (n_long) {
        StageTimer t(c, bm_write, long_bytes + n_long * 32 + bm_bits);
        HIPCHK(c, pm_launch_bitmap<true>(slab, bm_grid, bm_lds, st, A, order, n_long, slabs, sizes, nx->last_ids, nx->offsets, nx->value, err));
    }
    if (n_short) {
        StageTimer t(c, "permute_write_sort", ix->value_len - long_bytes + hv[0] + n_short * 28);
        hipLaunchKernelGGL((k_pm_sort<true>), dim3(fd_grid(n_short, PM_SORT_WAVES)), dim3(PM_SORT_WAVES * FD_WAVE), 0, st, A, order + n_long, n_short, sizes,
                           nx->last_ids, nx->offsets, nx->value, err);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));      // the result is complete, and the context's workspaces free again, when the call returns
    return FDGPU_OK;
}

extern "C" int fdgpu_index_permute(fdgpu_ctx *c, const fdgpu_index *ix, const uint32_t *new_id, uint64_t n, fdgpu_index **out) { FD_LOCK(c);
    if (!c || !ix || !out || (n && !new_id)) return FDGPU_EINVAL;
    *out = nullptr;
    if (n != ix->n_structures) FAIL(c, FDGPU_EINVAL, "index permute: n differs from the index's number of structures");
    {      // a permutation of 0 .. n - 1: every value below n, none twice
        std::vector<uint64_t> seen((n + 63) / 64, 0);
        for (uint64_t s = 0; s < n; ++s) {
            const uint64_t p = new_id[s];
            if (p >= n || (seen[p >> 6] >> (p & 63) & 1u)) FAIL(c, FDGPU_EINVAL, "index permute: new_id is not a permutation of 0 .. n - 1");
            seen[p >> 6] |= 1ull << (p & 63);
        }
    }
    fdgpu_index *nx = nullptr;
    const int rc = permute_impl(c, ix, new_id, &nx);
    if (rc != FDGPU_OK) return fd_index_op_failed(c, rc, &nx);
    *out = nx;
    return FDGPU_OK;
}
