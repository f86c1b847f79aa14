// k_verify.hip — fdgpu_index_verify: is a resident index well formed (fd_verify.h)?
//
//   k_vf_table   thread per slot 0 .. H: classes 1-3 from the offsets and hashes alone; the longest list; the slots of the lists of at least
//                VF_LONG_BYTES go to a queue
//   k_vf_lists   only behind a clean table (the offsets are addresses now): every value byte is decoded once.
//                  blocks 0 .. n_long / 4     a wavefront per queued long list, so that the longest walks start first instead of trailing
//                  the other blocks           256 slots each.  A list of at most 8 bytes is its own thread's: one 8-byte window, byte by byte.
//                                             Lists of 9 .. 128 bytes are shared out over the wavefront's eight groups of eight lanes, the
//                                             longer ones are walked by the whole wavefront one after the other.
//                A group of G lanes walks 4 G bytes per step, four per lane.  What a byte shows depends on the bytes before it only through
//                its position inside its varint, and that position matters up to five: a lane gets it from the trailing continuation bytes
//                of the words of the one or two lanes before it (across steps: of the last two lanes of the step before).  Classes 5-7 are
//                then per-byte predicates (fd_vf_byte, the code the host checker runs byte by byte), the list's last id is the sum over its
//                bytes of (byte & 0x7f) << 7 * position, the first id is the 8-byte window at the list's start.
// No address is formed from a decoded value; a lane loads its 4 bytes only if the first of them lies inside its list, so nothing beyond
// value_len + 3 is read (FD_VALUE_SLACK covers it and the 8-byte window).  Slots, classes and totals go to 16 counters in a context workspace:
// the lowest bad slot by one 64-bit atomicMin of slot << 8 | mask, so the report does not depend on scheduling.
#include "fdgpu_internal.h"
#include "fd_api_common.h"
#include "fd_postings.h"
#include "fd_verify.h"

#define VF_LONG_BYTES 16384u      // lists at least this long are walked first, by wavefronts of their own
#define VF_THREAD_BYTES 8u        // lists up to here: thread per list
#define VF_GROUP_BYTES 128u       // lists up to here: eight lanes per list
// counters: [0] min of slot << 8 | mask, [1] bad slots, [2..9] classes 1..8, [10] postings, [11] max id, [12] longest list, [13] queued long lists
#define VF_FIRST 0
#define VF_NBAD 1
#define VF_CLASS0 1
#define VF_POST 10
#define VF_MAXID 11
#define VF_MAXLEN 12
#define VF_NLONG 13

typedef unsigned long long vf_u64;

// every lane of the wavefront calls this with the mask of the slot it answers for (0: none or clean)
__device__ __forceinline__ void vf_tally(vf_u64 *__restrict__ cnt, uint64_t slot, uint32_t mask, uint32_t lane) {
    const uint64_t bad = __ballot(mask != 0u);
    if (!bad) return;
    const uint32_t leader = (uint32_t)__ffsll((long long)bad) - 1u;
    for (uint32_t c = 1; c <= 8; ++c) {
        const uint64_t b = __ballot((mask & FD_VF_BIT(c)) != 0u);
        if (b && lane == leader) atomicAdd(&cnt[VF_CLASS0 + c], (vf_u64)__popcll(b));
    }
    if (lane == leader) atomicAdd(&cnt[VF_NBAD], (vf_u64)__popcll(bad));
    if (mask) atomicMin(&cnt[VF_FIRST], (vf_u64)(slot << 8 | mask));
}
__device__ __forceinline__ uint64_t vf_wave_max(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) { const uint64_t u = __shfl_xor(v, o, FD_WAVE); v = u > v ? u : v; }
    return v;
}
__device__ __forceinline__ uint64_t vf_wave_sum(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, FD_WAVE);
    return v;
}

__global__ __launch_bounds__(256) void k_vf_table(const uint32_t *__restrict__ hashes, const uint64_t *__restrict__ offsets, uint64_t H, uint64_t value_len,
                                                  vf_u64 *__restrict__ cnt, uint32_t *__restrict__ long_q, uint64_t long_cap) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t m = 0;
    uint64_t len = 0;
    if (k <= H) {
        const uint64_t o0 = offsets[k];
        if (k == 0 && o0 != 0) m |= FD_VF_BIT(1);
        if (k == H && o0 != value_len) m |= FD_VF_BIT(1);
        if (k < H) {
            const uint64_t o1 = offsets[k + 1];
            if (!(o0 < o1 && o1 <= value_len)) m |= FD_VF_BIT(2);
            else len = o1 - o0;
        }
        if (k + 1 < H && !(hashes[k] < hashes[k + 1])) m |= FD_VF_BIT(3);
    }
    vf_tally(cnt, k, m, lane);
    if (len >= VF_LONG_BYTES) {
        const vf_u64 at = atomicAdd(&cnt[VF_NLONG], 1ull);
        if (at < long_cap) long_q[at] = (uint32_t)k;      // a clean table has at most value_len / VF_LONG_BYTES such lists and H <= 2^32
    }
    const uint64_t mx = vf_wave_max(len);
    if (lane == 0 && mx) atomicMax(&cnt[VF_MAXLEN], (vf_u64)mx);
}

struct vf_args { const uint64_t *offsets; const uint8_t *value; uint64_t H, value_len, first_id, limit; };
struct vf_acc { uint64_t post, max_id; };      // per lane, over the whole kernel

// G lanes (sub = 0 .. G - 1) walk the list b0 .. b1 (b0 >= b1: nothing).  -> the list's mask, valid in the group's lane 0
template <int G>
__device__ __forceinline__ uint32_t vf_walk(const vf_args &A, uint64_t b0, uint64_t b1, uint32_t sub, vf_acc *acc) {
    uint32_t cls = 0, nf = 0, n_term = 0;
    uint64_t sum = 0, first = 0;
    if (b0 < b1) first = fd_first_varint(A.value + b0, &nf);      // the same 8 bytes for every lane of the group
    uint32_t c1 = 0, c2 = 0;                                      // trailing continuation bytes | their value bits << 3 of the last two lanes of the step before
    uint64_t p = b0 + 4u * sub;
    uint32_t cur = 0, last_byte = 0;
    if (p < b1) __builtin_memcpy(&cur, A.value + p, 4);
    if (sub == 0 && b0 < b1) last_byte = A.value[b1 - 1];
    for (uint64_t base = b0; __ballot(base < b1) != 0ull; base += 4u * G) {      // the wavefront leaves the loop together: the shuffles inside stay whole
        p = base + 4u * sub;
        const uint64_t pn = p + 4u * G;
        uint32_t nxt = 0;
        if (pn < b1) __builtin_memcpy(&nxt, A.value + pn, 4);     // the next step's word, in flight while this one is decoded
        const uint32_t w = cur;
        const uint32_t n_in = p >= b1 ? 0u : (b1 - p >= 4u ? 4u : (uint32_t)(b1 - p));      // bytes of this lane inside the list
        // trailing continuation bytes of the word (0..4) and whether they hold value bits
        const uint32_t tc = n_in < 4u ? 0u : (uint32_t)__clz((int)(~w & 0x80808080u)) >> 3;      // a partial word is the list's last: nothing follows it
        const uint32_t tz = tc && ((w & 0x7f7f7f7fu) >> ((8u * (4u - tc)) & 31u)) ? 1u : 0u;
        const uint32_t t = tc | tz << 3;
        uint32_t t1 = __shfl_up(t, 1, G), t2 = __shfl_up(t, 2, G);
        if (sub == 0) { t1 = c1; t2 = c2; }
        if (sub == 1) t2 = c1;
        c1 = __shfl(t, G - 1, G); c2 = __shfl(t, G - 2, G);
        fd_vf_state s;
        const uint32_t tc1 = t1 & 7u, tc2 = t2 & 7u;
        s.pin = tc1 < 4u ? tc1 : (tc2 ? 5u : 4u);
        s.nz = tc1 < 4u ? t1 >> 3 : (t1 | t2) >> 3;
        uint64_t part = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (j < n_in) {
                uint64_t add;
                uint32_t term;
                cls |= fd_vf_byte(&s, (w >> (8u * j)) & 0xffu, p + j - b0 + 1u == nf, &add, &term);
                part += add;
                n_term += term;
            }
        sum = fd_vf_sat(sum + part);
        cur = nxt;
    }
    acc->post += n_term;
    for (int o = G / 2; o > 0; o >>= 1) {
        cls |= __shfl_xor(cls, o, G);
        sum = fd_vf_sat(sum + __shfl_xor(sum, o, G));
    }
    if (b0 >= b1) return 0u;
    const uint32_t m = fd_vf_list_mask(cls, last_byte, first, sum, A.first_id, A.limit);      // last_byte: lane 0's
    if (sub == 0 && !m) acc->max_id = sum > acc->max_id ? sum : acc->max_id;
    return m;
}

__device__ __forceinline__ void vf_flush(vf_u64 *__restrict__ cnt, const vf_acc &acc, uint32_t lane) {
    const uint64_t post = vf_wave_sum(acc.post), mx = vf_wave_max(acc.max_id);
    if (lane == 0) {
        if (post) atomicAdd(&cnt[VF_POST], (vf_u64)post);
        if (mx) atomicMax(&cnt[VF_MAXID], (vf_u64)mx);
    }
}

__global__ __launch_bounds__(256) void k_vf_lists(vf_args A, const uint32_t *__restrict__ long_q, uint64_t n_long, uint32_t long_blocks, vf_u64 *__restrict__ cnt) {
    const uint32_t lane = threadIdx.x & 63u;
    vf_acc acc = {0, 0};
    if (blockIdx.x < long_blocks) {      // a wavefront per long list
        const uint64_t g = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
        if (g >= n_long) return;
        const uint64_t k = long_q[g];
        uint64_t b0 = 0, b1 = 0;
        if (k < A.H) { b0 = A.offsets[k]; b1 = A.offsets[k + 1]; }
        if (!(b0 < b1 && b1 <= A.value_len)) b0 = b1 = 0;
        const uint32_t m = vf_walk<64>(A, b0, b1, lane, &acc);
        vf_tally(cnt, k, lane == 0 ? m : 0u, lane);
        vf_flush(cnt, acc, lane);
        return;
    }
    const uint64_t k = ((uint64_t)(blockIdx.x - long_blocks) * 256u) + threadIdx.x;
    const uint64_t wave_k0 = k - lane;
    uint64_t b0 = 0, b1 = 0;
    if (k < A.H) { b0 = A.offsets[k]; b1 = A.offsets[k + 1]; }
    if (!(b0 < b1 && b1 <= A.value_len)) b0 = b1 = 0;             // cannot happen behind a clean table; the walk must not depend on that
    const uint64_t len = b1 - b0;
    // 1. thread per list
    {
        const bool mine = len && len <= VF_THREAD_BYTES;
        uint32_t m = 0;
        if (mine) {
            unsigned long long w;
            __builtin_memcpy(&w, A.value + b0, 8);
            fd_vf_state s = {0, 0};
            uint32_t cls = 0, n_term = 0;
            uint64_t sum = 0, first = 0;
#pragma unroll
            for (uint32_t j = 0; j < VF_THREAD_BYTES; ++j)
                if (j < len) {
                    uint64_t add;
                    uint32_t term;
                    cls |= fd_vf_byte(&s, (uint32_t)(w >> (8u * j)) & 0xffu, n_term == 0, &add, &term);
                    sum += add;
                    if (n_term == 0) first += add;
                    n_term += term;
                }
            acc.post += n_term;
            m = fd_vf_list_mask(cls, (uint32_t)(w >> (8u * (len - 1))) & 0xffu, first, sum, A.first_id, A.limit);
            if (!m) acc.max_id = sum > acc.max_id ? sum : acc.max_id;
        }
        vf_tally(cnt, k, m, lane);
    }
    // 2. eight lanes per list: group g takes the g-th waiting list of the round
    uint64_t wait = __ballot(len > VF_THREAD_BYTES && len <= VF_GROUP_BYTES);
    const uint32_t grp = lane >> 3, sub = lane & 7u;
    while (wait) {
        uint32_t src = 64;
        for (uint32_t g = 0; g < 8 && wait; ++g) {
            const uint32_t s = (uint32_t)__ffsll((long long)wait) - 1u;
            wait &= wait - 1ull;
            if (grp == g) src = s;
        }
        uint64_t g0 = __shfl(b0, src & 63u, FD_WAVE), g1 = __shfl(b1, src & 63u, FD_WAVE);
        if (src == 64) g0 = g1 = 0;
        const uint32_t m = vf_walk<8>(A, g0, g1, sub, &acc);
        vf_tally(cnt, wave_k0 + src, sub == 0 && src < 64 ? m : 0u, lane);
    }
    // 3. the wavefront per list
    wait = __ballot(len > VF_GROUP_BYTES && len < VF_LONG_BYTES);
    while (wait) {
        const uint32_t src = (uint32_t)__ffsll((long long)wait) - 1u;
        wait &= wait - 1ull;
        const uint64_t g0 = __shfl(b0, src, FD_WAVE), g1 = __shfl(b1, src, FD_WAVE);
        const uint32_t m = vf_walk<64>(A, g0, g1, lane, &acc);
        vf_tally(cnt, wave_k0 + src, lane == 0 ? m : 0u, lane);
    }
    vf_flush(cnt, acc, lane);
}

extern "C" int fdgpu_index_verify(fdgpu_ctx *c, const fdgpu_index *ix, fd_verify_report *report) { FD_LOCK(c);
    if (!c || !ix || !report) return FDGPU_EINVAL;
    reset_timings(c);
    hipStream_t st = c->stream;
    const uint64_t H = ix->n_hashes, V = ix->value_len;
    const uint64_t long_cap = V / VF_LONG_BYTES + 1;
    HIPCHK(c, c->ws[WS_MISC0].ensure(16 * 8));
    HIPCHK(c, c->ws[WS_MISC1].ensure(long_cap * 4));
    vf_u64 *cnt = c->ws[WS_MISC0].as<vf_u64>();
    uint32_t *long_q = c->ws[WS_MISC1].as<uint32_t>();
    uint64_t h[16] = {0};
    h[VF_FIRST] = ~0ull;
    HIPCHK(c, hipMemcpyAsync(cnt, h, sizeof h, hipMemcpyHostToDevice, st));
    {
        StageTimer t(c, "verify_table", H * 12 + 8);
        hipLaunchKernelGGL(k_vf_table, dim3(fd_grid(H + 1, 256)), dim3(256), 0, st, ix->hashes, ix->offsets, H, V, cnt, long_q, long_cap);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h, cnt, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const bool lists = h[VF_NBAD] == 0;
    if (lists && H) {
        const uint64_t n_long = std::min<uint64_t>(h[VF_NLONG], long_cap);
        const uint32_t long_blocks = fd_grid(n_long, 4);
        const vf_args A = {ix->offsets, ix->value, H, V, ix->first_id, fd_vf_id_limit(ix->first_id, ix->n_structures)};
        {
            StageTimer t(c, "verify_lists", V + H * 8);
            hipLaunchKernelGGL(k_vf_lists, dim3(long_blocks + fd_grid(H, 256)), dim3(256), 0, st, A, long_q, n_long, long_blocks, cnt);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h, cnt, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    uint32_t first_hash = 0;
    uint64_t first_offset = 0;
    if (h[VF_NBAD]) {
        const uint64_t slot = h[VF_FIRST] >> 8;
        if (slot < H) HIPCHK(c, hipMemcpyAsync(&first_hash, ix->hashes + slot, 4, hipMemcpyDeviceToHost, st));
        if (slot <= H) HIPCHK(c, hipMemcpyAsync(&first_offset, ix->offsets + slot, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    fd_vf_fill_report(report, h, H, lists, first_hash, first_offset);
    return FDGPU_OK;
}
