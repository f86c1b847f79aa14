// k_merge.hip — device-side merge of resident sub-indices into ONE resident index.
//
// A shard with more than 2^32 residue pairs is built as several fdgpu_index_build calls over consecutive structure-id
// ranges (controller/mod.rs:282-348 walks the input in chunks in the same way).  The reference ends with one table per hash
// whose posting list is the concatenation of the chunks' lists (ids ascending: indextable.rs:171-202 appends in id order).
// Here every chunk is a complete sub-index, so the single index is, per hash, the concatenation of the parts' byte strings
// with the first varint of every continuation re-based from "absolute id" to "delta from the previous part's last id".
//
//   union of the parts' hash sets    bitmap over the hash space (2^30 bits, 2^32 when a part holds an overflowed hash) +
//                                    popcount prefix -> rank(h) = merged slot; coalesced, no sort
//   slot -> position in every part   pos[slot][part] (u32, NONE = absent), filled by one pass over each part's hashes
//   sizes                            thread per merged slot: byte lengths from the parts' offsets, the re-based head from the part's
//                                    first varint and the previous part's LAST id (the encoder stores one u32 per list; for a
//                                    loaded index k_mg_last_ids sums (byte & 0x7f) << 7 * (position inside its varint) over the list)
//   copy                             one wavefront per merged slot, eight lanes per part, 16 bytes per lane and step
// HBM-bound byte work: one read + one write of the value bytes.
#include "fdgpu_internal.h"
#include "fd_api_common.h"
#include "fd_postings.h"

#define MG_NONE 0xffffffffu
#define MG_MAX_PARTS 64

struct mg_part { const uint32_t *hashes; const uint64_t *offsets; const uint8_t *value; const uint32_t *last_ids; uint64_t H; };

__global__ void k_mg_bitmap_set(const uint32_t *__restrict__ hashes, uint64_t n, uint32_t *__restrict__ bitmap) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t h = hashes[t];
    atomicOr(&bitmap[h >> 5], 1u << (h & 31u));
}
__global__ void k_mg_popc(const uint32_t *__restrict__ bitmap, uint64_t n_words, uint32_t *__restrict__ cnt) {
    uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < n_words) cnt[w] = (uint32_t)__popc(bitmap[w]);
}
__global__ void k_mg_expand(const uint32_t *__restrict__ bitmap, const uint64_t *__restrict__ prefix, uint64_t n_words, uint32_t *__restrict__ out) {
    uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint32_t m = bitmap[w];
    uint64_t p = prefix[w];
    while (m) {
        const uint32_t b = (uint32_t)__ffs(m) - 1u;
        out[p++] = (uint32_t)(w << 5) | b;
        m &= m - 1u;
    }
}
__global__ void k_mg_pos_fill(const uint32_t *__restrict__ hashes, uint64_t n, const uint32_t *__restrict__ bitmap, const uint64_t *__restrict__ prefix,
                              uint32_t *__restrict__ pos, uint32_t part, uint32_t n_parts) {
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t h = hashes[t];
    const uint64_t g = prefix[h >> 5] + (uint32_t)__popc(bitmap[h >> 5] & ((1u << (h & 31u)) - 1u));
    pos[g * n_parts + part] = (uint32_t)t;
}

// last structure id of every list of an index that carries no last_ids (fdgpu_index_load): one wavefront per list, the last id is
// the sum over the list's bytes of (byte & 0x7f) << 7 * (position inside its varint)
__global__ __launch_bounds__(256) void k_mg_last_ids(const uint64_t *__restrict__ offsets, const uint8_t *__restrict__ value, uint64_t H, uint32_t *__restrict__ last_ids) {
    const uint64_t t = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= H) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t b0 = offsets[t], b1 = offsets[t + 1];
    uint32_t acc = 0, carry = 0;
    for (uint64_t base = b0; base < b1; base += FD_WAVE) {
        const uint64_t p = base + lane;
        const bool in = p < b1;
        const uint32_t byte = in ? value[p] : 0x80u;
        const uint64_t tm = __ballot(in && !(byte & 0x80u));
        const uint64_t below = tm & ((1ull << lane) - 1ull);
        const uint32_t pin = below ? lane - (uint32_t)(63 - __clzll(below)) - 1u : lane + carry;
        acc += in ? (byte & 0x7fu) << (7u * (pin < 5u ? pin : 4u)) : 0u;
        carry = tm ? 63u - (uint32_t)(63 - __clzll(tm)) : carry + 64u;
    }
    acc = fd_wave_sum(acc);
    if (lane == 0) last_ids[t] = acc;
}

// sizes: thread = merged slot.  size = sum over the parts holding the hash of (bytes of the part's list), the first varint of every
// continuation re-based from "absolute id" to "delta from the previous part's last id"
// One thread per merged slot walks the parts that hold its hash: byte size of the merged list (a continuation's first varint shrinks from
// an absolute id to a delta against the previous part's last id) and a COPY PLAN per (slot, part) — source offset of the bytes that move
// verbatim, their count, the re-encoded first value and where the piece starts inside the merged list — so that the copy kernel's pieces
// are independent of each other and sit behind ONE dependent load instead of four (position table -> offsets -> first varint -> bytes).
struct mg_plan { uint32_t src_lo, src_hi_dl, n, delta; };      // src_hi_dl: bits 0-15 source offset >> 32, bits 16-18 varint length, bit 31 present
__global__ __launch_bounds__(256) void k_mg_sizes(const mg_part *__restrict__ parts, uint32_t n_parts, const uint32_t *__restrict__ pos, uint64_t n_slots,
                                                  uint32_t *__restrict__ sizes, uint32_t *__restrict__ out_last, mg_plan *__restrict__ plan,
                                                  uint32_t *__restrict__ plan_dst, uint32_t *__restrict__ err_flag) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_slots) return;
    uint32_t total = 0, prev_last = 0;
    bool have_prev = false;
    for (uint32_t k = 0; k < n_parts; ++k) {
        const uint32_t t = pos[g * n_parts + k];
        mg_plan pl = {0u, 0u, 0u, 0u};
        if (t != MG_NONE) {
            const mg_part P = parts[k];
            const uint64_t b0 = P.offsets[t], b1 = P.offsets[t + 1];
            uint32_t len = (uint32_t)(b1 - b0), nf = 0, dl = 0, delta = 0;
            if (b1 - b0 > 0xffffffffull - total) *err_flag = 1u;      // a merged list of 4 GiB or more does not fit the u32 plan: the call fails (FDGPU_ERANGE)
            if (have_prev) {
                const uint32_t first = fd_first_varint(P.value + b0, &nf);
                delta = first - prev_last;
                dl = fd_varint_len(delta);
                len = len - nf + dl;
            }
            const uint64_t src = b0 + nf;
            pl.src_lo = (uint32_t)src; pl.src_hi_dl = (uint32_t)(src >> 32) | (dl << 16) | 0x80000000u; pl.n = len - dl; pl.delta = delta;
            plan_dst[g * n_parts + k] = total;
            total += len;
            prev_last = P.last_ids[t];
            have_prev = true;
        }
        plan[g * n_parts + k] = pl;
    }
    sizes[g] = total;
    out_last[g] = prev_last;
}

// copy: eight lanes per (slot, part) piece (fd_list_copy); the pieces of one slot are adjacent work items, so a merged list still leaves through
// neighbouring lanes
__global__ __launch_bounds__(256) void k_mg_copy(const mg_part *__restrict__ parts, uint32_t n_parts, const mg_plan *__restrict__ plan,
                                                 const uint32_t *__restrict__ plan_dst, uint64_t n_pieces, const uint64_t *__restrict__ out_off,
                                                 uint8_t *__restrict__ out_value) {
    const uint64_t G = (uint64_t)blockIdx.x * 32u + (threadIdx.x >> 3);
    if (G >= n_pieces) return;
    const mg_plan pl = plan[G];
    if (!(pl.src_hi_dl & 0x80000000u)) return;
    const uint32_t sub = threadIdx.x & 7u, k = (uint32_t)(G % n_parts);
    const uint64_t slot = G / n_parts;
    const uint32_t dl = (pl.src_hi_dl >> 16) & 7u;
    const uint8_t *sp = parts[k].value + (((uint64_t)(pl.src_hi_dl & 0xffffu) << 32) | pl.src_lo);
    fd_list_copy(out_value + out_off[slot] + plan_dst[G], pl.delta, dl, sp, pl.n, sub);
}

// the last id of every list of ix, once: an index that was loaded carries none.  Derived like lens (fd_api_count.hip): made under lens_mu and
// complete before it is published, because sibling contexts (query lanes) may share the index and read it from their own streams
int fd_index_last_ids(fdgpu_ctx *c, const fdgpu_index *ix) {
    std::lock_guard<std::mutex> lk(ix->lens_mu);
    if (ix->last_ids || !ix->n_hashes) return FDGPU_OK;
    uint32_t *l = nullptr;
    HIPCHK(c, hipMalloc((void **)&l, ix->n_hashes * 4));
    hipLaunchKernelGGL(k_mg_last_ids, dim3(fd_grid(ix->n_hashes, 4)), dim3(256), 0, c->stream, ix->offsets, ix->value, ix->n_hashes, l);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(l); c->err = std::string("last ids of the index: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    ix->last_ids = l;
    return FDGPU_OK;
}

extern "C" int fdgpu_index_merge(fdgpu_ctx *c, const fdgpu_index *const *parts, uint64_t n_parts, fdgpu_index **out) { FD_LOCK(c);
    if (!c || !out || !n_parts || !parts) return FDGPU_EINVAL;
    *out = nullptr;
    if (n_parts > MG_MAX_PARTS) FAIL(c, FDGPU_ERANGE, "index merge: at most 64 parts per call (merge in rounds)");
    reset_timings(c);
    hipStream_t st = c->stream;
    uint64_t n_struct = 0, n_post = 0, sum_h = 0, sum_v = 0;
    std::vector<mg_part> ph(n_parts);
    for (uint64_t k = 0; k < n_parts; ++k) {
        const fdgpu_index *p = parts[k];
        if (!p) return FDGPU_EINVAL;
        if (k && p->first_id != parts[k - 1]->first_id + parts[k - 1]->n_structures)
            FAIL(c, FDGPU_EINVAL, "index merge: parts must cover consecutive structure-id ranges in the order given");
        if (int rc = fd_index_last_ids(c, p)) return rc;
        ph[k] = {p->hashes, p->offsets, p->value, p->last_ids, p->n_hashes};
        n_struct += p->n_structures; n_post += p->n_postings; sum_h += p->n_hashes; sum_v += p->value_len;
    }
    // hash space: 2^30 unless a part holds an overflowed hash (unmasked OR of the fields)
    uint32_t max_hash = 0;
    for (uint64_t k = 0; k < n_parts; ++k)
        if (parts[k]->n_hashes) {
            uint32_t h = 0;
            HIPCHK(c, hipMemcpyAsync(&h, parts[k]->hashes + parts[k]->n_hashes - 1, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            max_hash = std::max(max_hash, h);
        }
    const uint64_t n_words = max_hash < (1u << 30) ? (1ull << 25) : (1ull << 27);
    HIPCHK(c, c->ws[WS_KEYS_A].ensure(n_words * 4));
    HIPCHK(c, c->ws[WS_KEYS_B].ensure(n_words * 4));
    HIPCHK(c, c->ws[WS_IDS_A].ensure((n_words + 2) * 8));
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(std::max<uint64_t>(n_words, sum_h)) * 8 + 64));
    HIPCHK(c, c->ws[WS_TOTAL].ensure(64));
    HIPCHK(c, c->ws[WS_MISC4].ensure(n_parts * sizeof(mg_part)));
    uint32_t *bitmap = c->ws[WS_KEYS_A].as<uint32_t>(), *cnt = c->ws[WS_KEYS_B].as<uint32_t>();
    uint64_t *prefix = c->ws[WS_IDS_A].as<uint64_t>();
    uint64_t Ht = 0;
    {
        StageTimer t(c, "merge_union", sum_h * 4 + n_words * 24);
        HIPCHK(c, hipMemsetAsync(bitmap, 0, n_words * 4, st));
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC4].p, ph.data(), n_parts * sizeof(mg_part), hipMemcpyHostToDevice, st));
        for (uint64_t k = 0; k < n_parts; ++k)
            if (ph[k].H) hipLaunchKernelGGL(k_mg_bitmap_set, dim3(fd_grid(ph[k].H, 256)), dim3(256), 0, st, ph[k].hashes, ph[k].H, bitmap);
        hipLaunchKernelGGL(k_mg_popc, dim3(fd_grid(n_words, 256)), dim3(256), 0, st, bitmap, n_words, cnt);
        fd_exclusive_scan<uint32_t>(cnt, n_words, prefix, c->ws[WS_SCANTMP].as<uint64_t>(), c->ws[WS_TOTAL].as<uint64_t>(), st);
    }
    HIPCHK(c, hipGetLastError());
    int rc = d2h_u64(c, c->ws[WS_TOTAL].as<uint64_t>(), &Ht);
    if (rc) return rc;
    fdgpu_index *ix = nullptr;
    if ((rc = fd_index_new(c, true, Ht, FD_VALUE_LATER, true, &ix))) return rc;
    ix->n_postings = n_post; ix->n_structures = n_struct; ix->first_id = parts[0]->first_id;
    hipError_t e = c->ws[WS_IDS_B].ensure(std::max<uint64_t>(Ht, 1) * n_parts * 4);
    if (e == hipSuccess) e = c->ws[WS_MISC0].ensure(std::max<uint64_t>(Ht, 1) * 4);
    if (e == hipSuccess) e = c->ws[WS_FRAMES].ensure(std::max<uint64_t>(Ht, 1) * n_parts * 16);     // copy plan: 16 + 4 bytes per (slot, part)
    if (e == hipSuccess) e = c->ws[WS_MISC1].ensure(std::max<uint64_t>(Ht, 1) * n_parts * 4);
    if (e != hipSuccess) { c->err = std::string("index merge alloc: ") + hipGetErrorString(e); fdgpu_index_destroy(ix); return FDGPU_EHIP; }
    uint32_t *pos = c->ws[WS_IDS_B].as<uint32_t>(), *sizes = c->ws[WS_MISC0].as<uint32_t>();
    {
        StageTimer t(c, "merge_sizes", sum_v + sum_h * 20 + Ht * n_parts * 8 + Ht * 16);
        hipLaunchKernelGGL(k_mg_expand, dim3(fd_grid(n_words, 256)), dim3(256), 0, st, bitmap, prefix, n_words, ix->hashes);
        (void)hipMemsetAsync(pos, 0xff, std::max<uint64_t>(Ht, 1) * n_parts * 4, st);
        for (uint64_t k = 0; k < n_parts; ++k)
            if (ph[k].H) hipLaunchKernelGGL(k_mg_pos_fill, dim3(fd_grid(ph[k].H, 256)), dim3(256), 0, st, ph[k].hashes, ph[k].H, bitmap, prefix, pos, (uint32_t)k, (uint32_t)n_parts);
        (void)hipMemsetAsync(c->ws[WS_TOTAL].as<uint32_t>() + 4, 0, 4, st);      // "a merged list does not fit 32 bits" flag, behind the scan total
        if (Ht) hipLaunchKernelGGL(k_mg_sizes, dim3(fd_grid(Ht, 256)), dim3(256), 0, st, c->ws[WS_MISC4].as<mg_part>(), (uint32_t)n_parts, pos, Ht, sizes,
                                   ix->last_ids, c->ws[WS_FRAMES].as<mg_plan>(), c->ws[WS_MISC1].as<uint32_t>(), c->ws[WS_TOTAL].as<uint32_t>() + 4);
        fd_exclusive_scan<uint32_t>(sizes, Ht, ix->offsets, c->ws[WS_SCANTMP].as<uint64_t>(), c->ws[WS_TOTAL].as<uint64_t>(), st);
    }
    e = hipGetLastError();
    uint64_t vlen = 0;
    if (e == hipSuccess) { rc = d2h_u64(c, c->ws[WS_TOTAL].as<uint64_t>(), &vlen); if (rc) { fdgpu_index_destroy(ix); return rc; } }
    if (e == hipSuccess) {
        uint32_t too_long = 0;
        e = hipMemcpy(&too_long, c->ws[WS_TOTAL].as<uint32_t>() + 4, 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && too_long) { fdgpu_index_destroy(ix); FAIL(c, FDGPU_ERANGE, "index merge: a merged posting list reaches 4 GiB"); }
    }
    if (e == hipSuccess) { ix->value_len = vlen; e = fd_index_block(c, vlen + FD_VALUE_SLACK, (void **)&ix->value, &ix->cap_value); }
    if (e != hipSuccess) { c->err = std::string("index merge: ") + hipGetErrorString(e); fdgpu_index_destroy(ix); return FDGPU_EHIP; }
    {
        StageTimer t(c, "merge_copy", sum_v + vlen + Ht * n_parts * 4);
        if (Ht) hipLaunchKernelGGL(k_mg_copy, dim3(fd_grid(Ht * n_parts, 32)), dim3(256), 0, st, c->ws[WS_MISC4].as<mg_part>(), (uint32_t)n_parts,
                                   c->ws[WS_FRAMES].as<mg_plan>(), c->ws[WS_MISC1].as<uint32_t>(), Ht * n_parts, ix->offsets, ix->value);
    }
    e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("index merge copy: ") + hipGetErrorString(e); fdgpu_index_destroy(ix); return FDGPU_EHIP; }
    *out = ix;
    return FDGPU_OK;
}

