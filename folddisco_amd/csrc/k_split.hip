// k_split.hip — device-side cut of a resident index by structure id range (fdgpu_index_split): the inverse of fdgpu_index_merge.
//
// Part r of W holds, for every hash, the ids in [bounds[r], bounds[r + 1]) with the ids unchanged, so it must equal a build over those structures
// with first_id = bounds[r] byte for byte.  Per posting list (first id f, last id l, part(x) = number of inner bounds <= x):
//
//   part(f) == part(l)     VERBATIM: the list moves as it is into that part
//   otherwise              CROSSING: every element whose part differs from its predecessor's is a piece head; a piece is the source bytes from
//                          its head to the next head with only the head varint rewritten from a delta to the absolute id (the inverse of the
//                          re-base in k_mg_copy)
//
//   k_sp_plan         thread per list: head, last id, their parts, class, long-first order key
//   order             crossing lists in the order the decode kernels take them (long ones first: fd_order_long_first, shared with k_prune.hip
//                     and k_permute.hip) and each list's place in it
//   k_sp_count        sizes pass over the VERBATIM lists, eight lanes per list: postings (terminator bytes), bytes and lists per part
//   k_sp_cross<W>     wavefront per CROSSING list, 256 bytes per step (fd_decode_step; its own copy of the walk, see there): W = 0 bytes / postings / last id of every piece (lane r
//                     keeps part r), W = 1 writes the pieces
//   k_sp_cross_totals the crossing pieces' bytes / postings / lists per part
//   per part:         k_sp_part_sizes -> two scans (slots, value offsets) -> k_sp_place (hashes / offsets / last ids at their slots, and where
//                     every list or piece of the part goes)
//   k_sp_copy         eight lanes per VERBATIM list (fd_list_copy)
// HBM-bound byte work: the value bytes are read twice (sizes, write) and written once; per part 30 bytes per hash of tables.
// Workspace: 40 bytes per list + 12 bytes per (crossing list, part) — see DESIGN.md §4b.
#include "fdgpu_internal.h"
#include "fd_api_common.h"
#include "fd_postings.h"

#define SP_MAX_PARTS 64u
#define SP_PF_BAD 0xffu           // plan: the list holds an id outside the index's range (the call fails before anything is written)
#define SP_TOT_BLOCKS 2048u       // blocks of the two totals kernels (each flushes its LDS histogram once)

struct sp_args { const uint64_t *offsets; const uint8_t *value; const uint32_t *last_ids; uint64_t H; uint64_t S; uint32_t first_id; uint32_t n_parts; };
struct sp_out { uint8_t *value; uint32_t *hashes; uint64_t *offsets; uint32_t *last_ids; };

// cuts[k] = bounds[k + 1] for k < n_parts - 1, 0xffffffff behind them (63 entries used): part(id) = number of cuts <= id, six branch-free steps
__device__ __forceinline__ uint32_t sp_part(const uint32_t *cuts, uint32_t id) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t s = 32; s; s >>= 1) pos += cuts[pos + s - 1] <= id ? s : 0u;
    return pos;
}
__device__ __forceinline__ void sp_load_cuts(uint32_t *lds, const uint32_t *__restrict__ cuts_g) {
    if (threadIdx.x < 64) lds[threadIdx.x] = cuts_g[threadIdx.x];
    __syncthreads();
}

// ---- plan: thread per list
__global__ __launch_bounds__(256) void k_sp_plan(sp_args A, const uint32_t *__restrict__ cuts_g, uint8_t *__restrict__ pf, uint8_t *__restrict__ cross,
                                                 uint8_t *__restrict__ is_long, uint32_t *__restrict__ err) {
    __shared__ uint32_t cuts[64];
    sp_load_cuts(cuts, cuts_g);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.H) return;
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    uint32_t nf = 0;
    const uint32_t f = fd_first_varint(A.value + b0, &nf), l = A.last_ids[t];
    uint32_t p = SP_PF_BAD, x = 0;
    if (b1 - b0 > 0xffffffffull) atomicOr(err, FD_IXERR_LONG);           // a list of 4 GiB or more: FDGPU_ERANGE
    if (b1 <= b0 || f < A.first_id || l < f || (uint64_t)l - A.first_id >= A.S) atomicOr(err, FD_IXERR_DAMAGED);
    else { p = sp_part(cuts, f); x = sp_part(cuts, l) != p ? 1u : 0u; }
    pf[t] = (uint8_t)p;
    cross[t] = (uint8_t)x;
    is_long[t] = (x && b1 - b0 >= FD_LONG_LIST_BYTES) ? 1u : 0u;
}

// per-part totals of a block: [0] lists, [1] bytes, [2] postings; one global atomic per non-zero entry when the block ends
__device__ __forceinline__ void sp_hist_flush(unsigned long long (*h)[64], unsigned long long *__restrict__ tot) {
    __syncthreads();
    if (threadIdx.x < 192) {
        const unsigned long long v = h[threadIdx.x >> 6][threadIdx.x & 63u];
        if (v) atomicAdd(tot + threadIdx.x, v);
    }
}

// ---- sizes pass, VERBATIM lists: eight lanes per list count the terminator bytes, 16 bytes per lane and step
__global__ __launch_bounds__(256) void k_sp_count(sp_args A, const uint8_t *__restrict__ pf, const uint8_t *__restrict__ cross,
                                                  unsigned long long *__restrict__ tot) {
    __shared__ unsigned long long h[3][64];
    if (threadIdx.x < 192) h[threadIdx.x >> 6][threadIdx.x & 63u] = 0;
    __syncthreads();
    const uint32_t sub = threadIdx.x & 7u;
    const uint64_t n_iter = (A.H + 32ull * gridDim.x - 1) / (32ull * gridDim.x);
    for (uint64_t it = 0; it < n_iter; ++it) {
        const uint64_t t = (it * gridDim.x + blockIdx.x) * 32u + (threadIdx.x >> 3);
        uint32_t cnt = 0, p = SP_PF_BAD;
        uint64_t n = 0;
        if (t < A.H && !cross[t]) p = pf[t];
        if (p != SP_PF_BAD) {
            const uint64_t b0 = A.offsets[t];
            n = A.offsets[t + 1] - b0;
            const uint8_t *sp = A.value + b0;
            uint64_t o = (uint64_t)sub * 16u;
            for (; o + 16 <= n; o += 128) {
                fd_u32x4 v;
                __builtin_memcpy(&v, sp + o, 16);
                cnt += __popc(~v.x & 0x80808080u) + __popc(~v.y & 0x80808080u) + __popc(~v.z & 0x80808080u) + __popc(~v.w & 0x80808080u);
            }
            if (o < n) for (uint64_t z = o; z < n; ++z) cnt += sp[z] & 0x80u ? 0u : 1u;
        }
        cnt += __shfl_xor(cnt, 1, FD_WAVE); cnt += __shfl_xor(cnt, 2, FD_WAVE); cnt += __shfl_xor(cnt, 4, FD_WAVE);
        if (sub == 0 && p != SP_PF_BAD) {
            atomicAdd(&h[0][p], 1ull); atomicAdd(&h[1][p], (unsigned long long)n); atomicAdd(&h[2][p], (unsigned long long)cnt);
        }
    }
    sp_hist_flush(h, tot);
}

// ---- CROSSING lists: wavefront per list, 64 lanes x 4 bytes per step.  W = false: tab[g][r] = {bytes, postings} and clast[g][r] of the list's piece
// in part r (lane r keeps part r).  W = true: tab[g][r] holds, as one u64, where that piece starts in part r's value bytes; the pieces are written.
// This kernel keeps its own copy of the walk of fd_wave_walk (fd_postings.h) and its 64-bit max scans: through fd_wave_walk its write pass measured
// 0.8 % slower at 542,000 structures (profiles/index_ops_refactor_S542000.json; same operations, another branch layout), so it stays instruction
// for instruction what it was.  A change to fd_wave_walk's carries has to be made here as well.
template <bool W>
__global__ __launch_bounds__(256) void k_sp_cross(sp_args A, const uint32_t *__restrict__ cuts_g, const uint32_t *__restrict__ order, uint64_t n_cross,
                                                  uint2 *__restrict__ tab, uint32_t *__restrict__ clast, const sp_out *__restrict__ outs,
                                                  uint32_t *__restrict__ err) {
    __shared__ uint32_t cuts[64];
    sp_load_cuts(cuts, cuts_g);
    const uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (g >= n_cross) return;
    const uint32_t lane = threadIdx.x & 63u, NP = A.n_parts;
    const uint64_t t = order[g];
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    unsigned long long dstp = 0;      // W: lane r = first byte of the list's piece in part r
    if (W && lane < NP) dstp = (unsigned long long)(outs[lane].value + ((const uint64_t *)tab)[g * NP + lane]);
    uint32_t acc = 0, cnt = 0, lastid = 0;      // sizes: bytes, postings, last id of the piece in part `lane`
    uint32_t run_id = 0;          // id of the last element decoded so far (the list's head is absolute: 0 + head)
    uint32_t cur_part1 = 0;       // part + 1 of the last element so far, 0 = none yet
    uint32_t piece_pos = 0;       // bytes of that element's piece so far
    bool prev_term = true;        // the byte before the step's first one ends a varint (the list start counts as one)
    const uint64_t p0 = b0 + 4u * lane;
    uint32_t cur = p0 < b1 ? fd_load4(A.value + p0) : 0u;
    for (uint64_t base = b0; base < b1; base += 256) {
        const uint64_t p = base + 4u * lane, pn = p + 256;
        const uint32_t nxt = pn < b1 ? fd_load4(A.value + pn) : 0u;      // next step's word, in flight while this one is decoded
        fd_step s;
        fd_decode_step(cur, nxt, p, b1, lane, prev_term, &s);
        const uint32_t dinc = fd_wave_scan_add(s.dsum, lane);
        uint32_t id = run_id + dinc - s.dsum;       // id before this lane's first element
        uint32_t idj[4], pj[4], lane_last = 0;      // lane_last: part + 1 of the lane's last element
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            idj[j] = 0; pj[j] = 0;
            if ((s.sb >> j) & 1u) {
                id += s.d[j];
                idj[j] = id;
                if (!W && (id < A.first_id || (uint64_t)id - A.first_id >= A.S)) atomicOr(err, FD_IXERR_DAMAGED);
                pj[j] = min(sp_part(cuts, id), NP - 1u);
                lane_last = pj[j] + 1u;
            }
        }
        const uint32_t lmax = (uint32_t)fd_wave_scan_max<uint64_t>(lane_last, lane);
        uint32_t pred = __shfl_up(lmax, 1, FD_WAVE);      // part + 1 of the last element before this lane's (0: none)
        if (lane == 0) pred = 0;
        if (cur_part1 > pred) pred = cur_part1;
        // heads (part differs from the predecessor's) and the bytes every element takes in its piece
        uint32_t ln[4], hm = 0, lsum = 0, q = pred;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            ln[j] = 0;
            if ((s.sb >> j) & 1u) {
                if (!W && pj[j] + 1u < q) atomicOr(err, FD_IXERR_DAMAGED);      // ids that do not ascend: the write pass relies on ascending parts
                const bool head = pj[j] + 1u != q;
                hm |= (head ? 1u : 0u) << j;
                ln[j] = head ? fd_varint_len(idj[j]) : s.nf[j];
                lsum += ln[j];
                q = pj[j] + 1u;
            }
        }
        const uint32_t linc = fd_wave_scan_add(lsum, lane);
        const uint32_t m63 = __shfl(lmax, FD_WAVE - 1, FD_WAVE);      // part + 1 of the step's last element (0: the step starts no varint)
        if (!W) {
            // the step's elements lie in parts q_lo .. q_hi (ascending ids): one wave sum per part, lane q keeps it
            const uint32_t q_lo = cur_part1 ? cur_part1 - 1u : __shfl(pj[0], 0, FD_WAVE);
            for (uint32_t qq = q_lo; qq + 1u <= m63; ++qq) {
                uint32_t v = 0, mx = 0;
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if (((s.sb >> j) & 1u) && pj[j] == qq) { v += (ln[j] << 16) | 1u; mx = idj[j]; }
                for (int o = 32; o > 0; o >>= 1) {
                    v += __shfl_xor(v, o, FD_WAVE);
                    const uint32_t u = __shfl_xor(mx, o, FD_WAVE);
                    mx = u > mx ? u : mx;
                }
                if (lane == qq && (v & 0xffffu)) { acc += v >> 16; cnt += v & 0xffffu; lastid = mx; }
            }
        }
        // where the piece of every element begins, in bytes from the step's first output byte: behind the latest head at or before it
        // (h1 = that head's prefix + 1); without a head in the step so far, the open piece continues (piece_pos bytes before the step)
        uint32_t epfx[4], lane_head = 0, run = linc - lsum;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) { epfx[j] = run; run += ln[j]; if ((hm >> j) & 1u) lane_head = epfx[j] + 1u; }
        const uint32_t hmax = (uint32_t)fd_wave_scan_max<uint64_t>(lane_head, lane);
        if (W) {
            uint32_t h1 = __shfl_up(hmax, 1, FD_WAVE);
            if (lane == 0) h1 = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const bool on = (s.sb >> j) & 1u;
                if ((hm >> j) & 1u) h1 = epfx[j] + 1u;
                uint8_t *o = (uint8_t *)__shfl(dstp, (int)pj[j], FD_WAVE) + (h1 ? epfx[j] - (h1 - 1u) : piece_pos + epfx[j]);
                if (on) {
                    if ((hm >> j) & 1u) {
                        fd_varint_store(o, idj[j], ln[j]);
                    } else {
                        const unsigned long long src = s.win >> (8 * j);
                        for (uint32_t b = 0; b < ln[j]; ++b) o[b] = (uint8_t)(src >> (8 * b));
                    }
                }
            }
        }
        // carries into the next step
        const uint32_t total = __shfl(linc, FD_WAVE - 1, FD_WAVE), h63 = __shfl(hmax, FD_WAVE - 1, FD_WAVE);
        piece_pos = h63 ? total - (h63 - 1u) : piece_pos + total;
        if (m63) cur_part1 = m63;
        run_id += __shfl(dinc, FD_WAVE - 1, FD_WAVE);
        prev_term = (__shfl(s.tb, FD_WAVE - 1, FD_WAVE) >> 3) & 1u;
        cur = nxt;
    }
    if (!W && lane < NP) {
        tab[g * NP + lane] = make_uint2(acc, cnt);
        clast[g * NP + lane] = lastid;
    }
}

// ---- lists / bytes / postings per part of the crossing pieces
__global__ __launch_bounds__(256) void k_sp_cross_totals(const uint2 *__restrict__ tab, uint64_t n_entries, uint32_t n_parts,
                                                         unsigned long long *__restrict__ tot) {
    __shared__ unsigned long long h[3][64];
    if (threadIdx.x < 192) h[threadIdx.x >> 6][threadIdx.x & 63u] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_entries; i += 256ull * gridDim.x) {
        const uint2 e = tab[i];
        if (e.x) {
            const uint32_t r = (uint32_t)(i % n_parts);
            atomicAdd(&h[0][r], 1ull); atomicAdd(&h[1][r], (unsigned long long)e.x); atomicAdd(&h[2][r], (unsigned long long)e.y);
        }
    }
    sp_hist_flush(h, tot);
}

// ---- per part r: the bytes every list leaves in it
__global__ void k_sp_part_sizes(sp_args A, uint32_t r, const uint8_t *__restrict__ pf, const uint8_t *__restrict__ cross, const uint32_t *__restrict__ xidx,
                                const uint2 *__restrict__ tab, uint32_t *__restrict__ sizes, uint8_t *__restrict__ flag) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.H) return;
    uint32_t sz = 0;
    if (cross[t]) sz = tab[(uint64_t)xidx[t] * A.n_parts + r].x;
    else if (pf[t] == r) sz = (uint32_t)(A.offsets[t + 1] - A.offsets[t]);
    sizes[t] = sz;
    flag[t] = sz ? 1u : 0u;
}
// ---- per part r: its non-empty lists -> their slots (offsets[H_r] = the part's value length), and where the write pass puts them: a VERBATIM
// list's place in its part (dstoff[t]), a piece's place over its {bytes, postings} entry of tab
__global__ void k_sp_place(sp_args A, uint32_t r, const uint32_t *__restrict__ hashes, const uint8_t *__restrict__ cross, const uint32_t *__restrict__ xidx,
                           const uint32_t *__restrict__ sizes, const uint64_t *__restrict__ slot, const uint64_t *__restrict__ off_all,
                           const uint32_t *__restrict__ clast, uint2 *__restrict__ tab, uint64_t *__restrict__ dstoff, sp_out O) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) O.offsets[slot[A.H]] = off_all[A.H];
    if (t >= A.H || sizes[t] == 0) return;
    const uint64_t s = slot[t], o = off_all[t];
    O.hashes[s] = hashes[t];
    O.offsets[s] = o;
    if (cross[t]) {
        const uint64_t e = (uint64_t)xidx[t] * A.n_parts + r;
        O.last_ids[s] = clast[e];
        ((uint64_t *)tab)[e] = o;
    } else {
        O.last_ids[s] = A.last_ids[t];
        dstoff[t] = o;
    }
}

// ---- VERBATIM lists: eight lanes per list (fd_list_copy), the head moves with the bytes
__global__ __launch_bounds__(256) void k_sp_copy(sp_args A, const uint8_t *__restrict__ pf, const uint8_t *__restrict__ cross,
                                                 const uint64_t *__restrict__ dstoff, const sp_out *__restrict__ outs) {
    const uint64_t t = (uint64_t)blockIdx.x * 32u + (threadIdx.x >> 3);
    if (t >= A.H || cross[t]) return;
    const uint64_t b0 = A.offsets[t], b1 = A.offsets[t + 1];
    fd_list_copy(outs[pf[t]].value + dstoff[t], 0u, 0u, A.value + b0, b1 - b0, threadIdx.x & 7u);
}

static int split_impl(fdgpu_ctx *c, const fdgpu_index *ix, uint32_t NP, const uint64_t *bounds, std::vector<fdgpu_index *> &parts) {
    reset_timings(c);
    hipStream_t st = c->stream;
    const uint64_t H = ix->n_hashes;
    if (int rc = fd_index_last_ids_staged(c, ix, "split_last_ids")) return rc;
    const uint64_t Hx = std::max<uint64_t>(H, 1);
    HIPCHK(c, c->ws[WS_MISC4].ensure(256 + SP_MAX_PARTS * sizeof(sp_out)));     // cuts, then the parts' arrays
    HIPCHK(c, c->ws[WS_MISC2].ensure(Hx * 4 + 16));                 // part of the head, crossing flag, long flag, non-empty flag of one part
    HIPCHK(c, c->ws[WS_IDS_A].ensure((Hx + 1) * 8));                // crossing prefix, then slots of one part
    HIPCHK(c, c->ws[WS_IDS_B].ensure((Hx + 1) * 8));                // long prefix, then value offsets of one part
    HIPCHK(c, c->ws[WS_KEYS_A].ensure(Hx * 4));                     // order of the crossing lists
    HIPCHK(c, c->ws[WS_KEYS_B].ensure(Hx * 4));                     // every crossing list's place in it
    HIPCHK(c, c->ws[WS_MISC0].ensure(Hx * 4));                      // sizes of one part
    HIPCHK(c, c->ws[WS_MISC1].ensure(Hx * 8));                      // where a VERBATIM list goes in its part
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(Hx) * 8 + 64));
    HIPCHK(c, c->ws[WS_TOTAL].ensure(2048));                        // [0] scan total, [1] error bits, [2 ..] lists / bytes / postings per part (3 x 64)
    uint32_t *cuts_d = c->ws[WS_MISC4].as<uint32_t>();
    sp_out *outs_d = (sp_out *)(c->ws[WS_MISC4].as<uint8_t>() + 256);
    uint8_t *pf = c->ws[WS_MISC2].as<uint8_t>(), *cross = pf + Hx, *is_long = pf + 2 * Hx, *flag = pf + 3 * Hx;
    uint64_t *pre_a = c->ws[WS_IDS_A].as<uint64_t>(), *pre_b = c->ws[WS_IDS_B].as<uint64_t>();
    uint32_t *order = c->ws[WS_KEYS_A].as<uint32_t>(), *xidx = c->ws[WS_KEYS_B].as<uint32_t>(), *sizes = c->ws[WS_MISC0].as<uint32_t>();
    uint64_t *dstoff = c->ws[WS_MISC1].as<uint64_t>();
    uint64_t *scan_tmp = c->ws[WS_SCANTMP].as<uint64_t>(), *tot = c->ws[WS_TOTAL].as<uint64_t>();
    uint32_t *err = (uint32_t *)(tot + 1);
    unsigned long long *ptot = (unsigned long long *)(tot + 2);
    uint32_t cuts[64];
    for (uint32_t k = 0; k < 64; ++k) cuts[k] = k + 1 < NP ? (uint32_t)bounds[k + 1] : 0xffffffffu;
    sp_args A{ix->offsets, ix->value, ix->last_ids, H, ix->n_structures, (uint32_t)ix->first_id, NP};
    uint64_t n_cross = 0;
    {
        StageTimer t(c, "split_plan", H * 27);
        HIPCHK(c, hipMemcpyAsync(cuts_d, cuts, sizeof cuts, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(tot + 1, 0, 8 + 3 * 64 * 8, st));
        if (H) {
            hipLaunchKernelGGL(k_sp_plan, dim3(fd_grid(H, 256)), dim3(256), 0, st, A, cuts_d, pf, cross, is_long, err);
            fd_order_long_first(cross, is_long, H, pre_a, pre_b, scan_tmp, tot, order, xidx, st);
        }
    }
    HIPCHK(c, hipGetLastError());
    if (H) {
        HIPCHK(c, hipMemcpyAsync(&n_cross, pre_a + H, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    const uint64_t n_ent = n_cross * NP;
    HIPCHK(c, c->ws[WS_FRAMES].ensure(std::max<uint64_t>(n_ent, 1) * 8));      // per (crossing list, part): {bytes, postings}, then the piece's place
    HIPCHK(c, c->ws[WS_MISC3].ensure(std::max<uint64_t>(n_ent, 1) * 4));       // ... and the piece's last id
    uint2 *tab = c->ws[WS_FRAMES].as<uint2>();
    uint32_t *clast = c->ws[WS_MISC3].as<uint32_t>();
    {
        StageTimer t(c, "split_sizes", ix->value_len + H * 18 + n_ent * 20);
        if (H) hipLaunchKernelGGL(k_sp_count, dim3((unsigned)std::min<uint64_t>(fd_grid(H, 32), SP_TOT_BLOCKS)), dim3(256), 0, st, A, pf, cross, ptot);
        if (n_cross) {
            hipLaunchKernelGGL((k_sp_cross<false>), dim3(fd_grid(n_cross, 4)), dim3(256), 0, st, A, cuts_d, order, n_cross, tab, clast, (const sp_out *)nullptr, err);
            hipLaunchKernelGGL(k_sp_cross_totals, dim3((unsigned)std::min<uint64_t>(fd_grid(n_ent, 256), SP_TOT_BLOCKS)), dim3(256), 0, st, tab, n_ent, NP, ptot);
        }
    }
    HIPCHK(c, hipGetLastError());
    uint64_t hv[1 + 3 * 64];      // error bits, then lists / bytes / postings per part
    HIPCHK(c, hipMemcpyAsync(hv, tot + 1, sizeof hv, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const uint32_t eb = (uint32_t)hv[0];
    if (eb & FD_IXERR_LONG) FAIL(c, FDGPU_ERANGE, "index split: a posting list reaches 4 GiB");
    if (eb & FD_IXERR_DAMAGED) FAIL(c, FDGPU_EINVAL, "index split: the index holds ids outside [first_id, first_id + n_structures) or ids that do not ascend");
    std::vector<sp_out> oh(NP);
    uint64_t v_out = 0;
    for (uint32_t r = 0; r < NP; ++r) {
        fdgpu_index *p = nullptr;
        if (int rc = fd_index_new(c, true, hv[1 + r], hv[1 + 64 + r], true, &p)) return rc;
        parts[r] = p;
        p->n_postings = hv[1 + 128 + r]; p->first_id = bounds[r]; p->n_structures = bounds[r + 1] - bounds[r];
        oh[r] = {p->value, p->hashes, p->offsets, p->last_ids};
        v_out += p->value_len;
    }
    {
        StageTimer t(c, "split_write", ix->value_len + v_out + H * 11 + (uint64_t)NP * H * 30 + n_ent * 16);
        HIPCHK(c, hipMemcpyAsync(outs_d, oh.data(), NP * sizeof(sp_out), hipMemcpyHostToDevice, st));
        for (uint32_t r = 0; r < NP; ++r) {
            if (!H) { HIPCHK(c, hipMemsetAsync(oh[r].offsets, 0, 8, st)); continue; }
            hipLaunchKernelGGL(k_sp_part_sizes, dim3(fd_grid(H, 256)), dim3(256), 0, st, A, r, pf, cross, xidx, tab, sizes, flag);
            fd_exclusive_scan<uint8_t>(flag, H, pre_a, scan_tmp, tot, st);          // slots of the part's lists
            fd_exclusive_scan<uint32_t>(sizes, H, pre_b, scan_tmp, tot, st);        // their value offsets
            hipLaunchKernelGGL(k_sp_place, dim3(fd_grid(H, 256)), dim3(256), 0, st, A, r, ix->hashes, cross, xidx, sizes, pre_a, pre_b, clast, tab, dstoff, oh[r]);
        }
        if (H) hipLaunchKernelGGL(k_sp_copy, dim3(fd_grid(H, 32)), dim3(256), 0, st, A, pf, cross, dstoff, outs_d);
        if (n_cross)
            hipLaunchKernelGGL((k_sp_cross<true>), dim3(fd_grid(n_cross, 4)), dim3(256), 0, st, A, cuts_d, order, n_cross, tab, clast, outs_d, err);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));      // oh (host) is read by the copy above; the parts are complete when the call returns
    return FDGPU_OK;
}

extern "C" int fdgpu_index_split(fdgpu_ctx *c, const fdgpu_index *ix, uint32_t n_parts, const uint64_t *bounds, fdgpu_index **out) { FD_LOCK(c);
    if (!c || !ix || !out || !bounds || n_parts < 1 || n_parts > SP_MAX_PARTS) return FDGPU_EINVAL;
    for (uint32_t r = 0; r < n_parts; ++r) out[r] = nullptr;
    if (bounds[0] != ix->first_id || bounds[n_parts] != ix->first_id + ix->n_structures)
        FAIL(c, FDGPU_EINVAL, "index split: bounds must start at first_id and end at first_id + n_structures");
    for (uint32_t r = 0; r < n_parts; ++r)
        if (bounds[r] > bounds[r + 1]) FAIL(c, FDGPU_EINVAL, "index split: bounds must ascend");
    if (bounds[n_parts] > 0xffffffffull) FAIL(c, FDGPU_ERANGE, "structure ids exceed 32 bits");
    std::vector<fdgpu_index *> parts(n_parts, nullptr);
    const int rc = split_impl(c, ix, n_parts, bounds, parts);
    if (rc != FDGPU_OK) return fd_index_op_failed(c, rc, parts.data(), parts.size());
    for (uint32_t r = 0; r < n_parts; ++r) out[r] = parts[r];
    return FDGPU_OK;
}
