// fd_postings.h — the posting-list byte format, stated once for the encoder (k_index.hip), the device merge (k_merge.hip), the removal
// (k_prune.hip), the split (k_split.hip), the rebase (k_rebase.hip), the reorder (k_permute.hip), the rows (k_rows.hip), the checker's first
// varints (k_verify.hip) and the host merge (fdgpu_merge_subindices).  Its host-safe part — the varint writer and reader — is
// fd_postings_host.h, which the host forms of those operations (fd_split_host.cpp, fd_rebase_host.cpp, fd_permute_host.cpp, fd_rows_host.cpp)
// take without this header's HIP include.
//
// A posting list is the ascending ids of the structures that hold one hash, as LEB128 varints (7-bit groups, least significant first; bit 7
// set = another byte follows; 0 is one 0x00 byte; a u32 takes at most five bytes; codec of indextable.rs:93-99, 397-418).  The first varint
// of a list is the absolute id, every later one the delta from the id before it.  An index stores its lists back to back in one value array
// (offsets[k] = first byte of list k) followed by FD_VALUE_SLACK readable bytes, so that the 8-byte window of fd_first_varint at the start of
// any list, the last one included, stays inside the allocation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fd_postings_host.h"

#ifndef FD_WAVE                 // fd_device.h defines it; tools/check_varint_pack.cpp parses this header for the host without that one
#define FD_WAVE 64
#endif

#define FD_VALUE_SLACK 16      // bytes behind an index's value array: fd_first_varint reads 8 bytes at the start of a list of any length

// bytes of the varint of v: 1 + ilog2(v) / 7, 1 for 0
__host__ __device__ __forceinline__ uint32_t fd_varint_len(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return v == 0 ? 1u : 1u + (31u - (uint32_t)__clz(v)) / 7u;      // __clz, not __builtin_clz: the encoder's code is smaller with it
#else
    return v == 0 ? 1u : 1u + (31u - (uint32_t)__builtin_clz(v)) / 7u;
#endif
}

// the len = fd_varint_len(v) bytes of the varint of v in the low bytes of a word, continuation bits set, the bytes above them zero; no branch on v.
// The 7-bit groups spread to one byte each (byte 4 = v >> 28); the len - 1 bytes below the last one carry bit 7: 0x80808080 shifted down by the
// 5 - len bytes that carry none (a shift of 0 .. 40 bits, so len = 0 is defined too: with v = 0 it gives 0, the encoder's "nothing to write").
__host__ __device__ __forceinline__ uint64_t fd_varint_pack(uint32_t v, uint32_t len) {
    const uint32_t g = (v & 0x7fu) | (v & 0x3f80u) << 1 | (v & 0x1fc000u) << 2 | (v & 0xfe00000u) << 3;
    const uint32_t cont = (uint32_t)(0x80808080ull >> (40u - 8u * len));
    return (uint64_t)(v >> 28) << 32 | (g | cont);
}

// ---- one element of a "constant" tile of the encoder's MSD stream (k_index.hip, enc_b24::cst): the element and its predecessor share the
// bucket and hash[23:8], so their u32 key words k, pk (hash[7:0] << 24 | local id, pk <= k) carry all that tells them apart.  A list head is a
// change of the top byte — never decided by k - pk: pk = 0x01000005, k = 0x02000001 differ by 0x00fffffc, a head that looks like a delta.
__host__ __device__ __forceinline__ bool fd_const_is_head(uint32_t k, uint32_t pk) { return ((k ^ pk) >> 24) != 0; }
// bytes a delta d < 2^31 writes: 0 for 0 (a repeat of the predecessor), else fd_varint_len(d) = ceil(bits(d) / 7).  d << 1 | 1 has one bit
// more than d and is never 0, so the count of leading zeros needs no test for it; n / 7 = n * 37 >> 8 for the n <= 37 that occur.
__host__ __device__ __forceinline__ uint32_t fd_delta_len(uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t z = (uint32_t)__clz((int)(d << 1 | 1u));
#else
    const uint32_t z = (uint32_t)__builtin_clz(d << 1 | 1u);
#endif
    return (37u - z) * 37u >> 8;
}
// an element that is no head: the delta between the two words is the delta of the ids, exact because the top bytes are equal, and below 2^24
__host__ __device__ __forceinline__ uint32_t fd_const_delta(uint32_t k, uint32_t pk, uint32_t *len) {
    const uint32_t d = k - pk;
    *len = fd_delta_len(d);
    return d;
}
// a head: its absolute id
__host__ __device__ __forceinline__ uint32_t fd_const_head(uint32_t k, uint32_t first_id, uint32_t *len) {
    const uint32_t id = first_id + (k & 0xffffffu);
    *len = fd_varint_len(id);
    return id;
}
// the whole rule: is the element a head, the value it writes and its bytes.  The encoder runs fd_const_delta on every element and
// fd_const_head behind a test of the wavefront's heads; tools/check_enc_const.cpp compares this with the rule on full hashes and ids.
__host__ __device__ __forceinline__ bool fd_const_classify(uint32_t k, uint32_t pk, uint32_t first_id, uint32_t *value, uint32_t *len) {
    const bool head = fd_const_is_head(k, pk);
    *value = head ? fd_const_head(k, first_id, len) : fd_const_delta(k, pk, len);
    return head;
}

// value and byte length of the varint at the low end of an 8-byte window
__device__ __forceinline__ uint32_t fd_varint_at(unsigned long long w, uint32_t *nf) {
    const unsigned long long stop = ~w & 0x8080808080ull;            // terminator bits of the first five bytes
    const uint32_t n = (uint32_t)__ffsll((long long)stop) >> 3;      // 1-based byte index of the first terminator
    *nf = n;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) if (k < n) v |= (uint32_t)((w >> (8 * k)) & 0x7full) << (7 * k);
    return v;
}
// first varint of a list: value and byte length (reads 8 bytes at p: FD_VALUE_SLACK)
__device__ __forceinline__ uint32_t fd_first_varint(const uint8_t *__restrict__ p, uint32_t *nf) {
    unsigned long long w;
    __builtin_memcpy(&w, p, 8);
    return fd_varint_at(w, nf);
}

// A list moved to a new place with a new head: lane sub (0..7) of the eight lanes that copy it writes byte sub of the dl-byte varint of head
// (dl = 0: the head moves with the bytes), then the n bytes at sp follow behind the head, 16 bytes per lane and step (unaligned 16-byte global
// accesses are native on gfx950); the lane that reaches the ragged tail (< 16 bytes) copies it byte by byte.
typedef unsigned int fd_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void fd_list_copy(uint8_t *__restrict__ d, uint32_t head, uint32_t dl, const uint8_t *__restrict__ sp, uint64_t n, uint32_t sub) {
    if (sub < dl) d[sub] = (uint8_t)(((head >> (7u * sub)) & 0x7fu) | (sub + 1u < dl ? 0x80u : 0u));
    d += dl;
    uint64_t o = (uint64_t)sub * 16u;
    for (; o + 16 <= n; o += 128) {
        fd_u32x4 v;
        __builtin_memcpy(&v, sp + o, 16);
        __builtin_memcpy(d + o, &v, 16);
    }
    if (o < n) for (uint64_t z = o; z < n; ++z) d[z] = sp[z];
}

// the ln = fd_varint_len(v) bytes of the varint of v at o, byte by byte (ln = 0: nothing)
__device__ __forceinline__ void fd_varint_store(uint8_t *o, uint32_t v, uint32_t ln) {
    for (uint32_t b = 0; b < ln; ++b) { o[b] = (uint8_t)((v & 0x7fu) | (b + 1 < ln ? 0x80u : 0u)); v >>= 7; }
}

// is id one of the index's S structures first_id .. first_id + S - 1?  *loc = its local position (meaningless when not)
__device__ __forceinline__ bool fd_id_local(uint32_t id, uint32_t first_id, uint64_t S, uint64_t *loc) {
    *loc = (uint64_t)id - first_id;
    return id >= first_id && *loc < S;
}

// ---- wavefront reductions and inclusive scans
__device__ __forceinline__ uint32_t fd_wave_sum(uint32_t v) {
    for (int o = FD_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, FD_WAVE);
    return v;
}
__device__ __forceinline__ uint32_t fd_wave_max(uint32_t v) {
    for (int o = FD_WAVE / 2; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(v, o, FD_WAVE); v = u > v ? u : v; }
    return v;
}
__device__ __forceinline__ uint32_t fd_wave_scan_add(uint32_t v, uint32_t lane) {
    for (int o = 1; o < FD_WAVE; o <<= 1) { const uint32_t u = __shfl_up(v, o, FD_WAVE); if ((int)lane >= o) v += u; }
    return v;
}
template <class T>      // uint32_t or uint64_t
__device__ __forceinline__ T fd_wave_scan_max(T v, uint32_t lane) {
    for (int o = 1; o < FD_WAVE; o <<= 1) { const T u = __shfl_up(v, o, FD_WAVE); if ((int)lane >= o && u > v) v = u; }
    return v;
}

// ---- a wavefront's walk over one list, 256 bytes per step (four per lane).  fd_wave_walk: the removal (k_pr_recode), the reorder's SORT class
// (k_pm_sort) and the rows (k_rw_walk).  fd_decode_step alone, with carries of their own: the reorder's BITMAP class (k_pm_bitmap: eight wavefronts per step, ids through
// fd_lane_starts) and the split (k_sp_cross, which keeps a copy of fd_wave_walk's loop for its speed — see there)
__device__ __forceinline__ uint32_t fd_load4(const uint8_t *p) { uint32_t w; __builtin_memcpy(&w, p, 4); return w; }
// One step: w = the lane's four bytes at p (0 beyond the list's end b1), nxt = its four bytes of the next step, prev_term = the byte before the
// step's first one ends a varint (the list start counts as one).  Out: tb = terminator bits of the lane's bytes, sb = bytes that start a varint,
// d[j] / nf[j] = value and byte length of the varint starting at byte j (0 where none starts), dsum = the lane's sum of d, win = the lane's word
// and the next lane's (lane 63: the next step's first word), which every start decodes from.
struct fd_step { uint32_t tb, sb, d[4], nf[4], dsum; unsigned long long win; };
__device__ __forceinline__ void fd_decode_step(uint32_t w, uint32_t nxt, uint64_t p, uint64_t b1, uint32_t lane, bool prev_term, fd_step *s) {
    uint32_t inm = 0, tb = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const bool in = p + j < b1;
        inm |= (in ? 1u : 0u) << j;
        tb |= (in && !((w >> (8 * j)) & 0x80u) ? 1u : 0u) << j;
    }
    const uint32_t tb_prev = __shfl_up(tb, 1, FD_WAVE);
    const uint32_t before0 = lane ? (tb_prev >> 3) & 1u : (prev_term ? 1u : 0u);
    s->tb = tb;
    s->sb = ((tb << 1) | before0) & inm & 0xfu;
    uint32_t w_hi = __shfl_down(w, 1, FD_WAVE);
    const uint32_t n0 = __shfl(nxt, 0, FD_WAVE);
    if (lane == FD_WAVE - 1) w_hi = n0;
    s->win = ((unsigned long long)w_hi << 32) | w;
    s->dsum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        uint32_t nfj = 0;
        s->d[j] = (s->sb >> j) & 1u ? fd_varint_at(s->win >> (8 * j), &nfj) : 0u;
        s->nf[j] = (s->sb >> j) & 1u ? nfj : 0u;
        s->dsum += s->d[j];
    }
}
// g(j, id) for every byte j of the lane's four at which a varint starts, id = its absolute id, given the id before the lane's first element.
// The add sits inside the test on purpose: a step in which no lane starts a varint at byte j skips the whole body.
template <class G>
__device__ __forceinline__ void fd_lane_starts(const fd_step &s, uint32_t id, G &&g) {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if ((s.sb >> j) & 1u) { id += s.d[j]; g(j, id); }
}
// f(step, id before the lane's first element) for every step of the list at value[b0 .. b1), all 64 lanes of the wavefront together.  The walk owns what one step hands to the
// next: the next step's word (loaded while this one is decoded; lane 63's window ends in it), whether the byte before the step ends a varint (one
// that straddles the step edge starts in this step and ends in the next), and the id of the last element so far.
template <class F>
__device__ __forceinline__ void fd_wave_walk(const uint8_t *__restrict__ value, uint64_t b0, uint64_t b1, uint32_t lane, F &&f) {
    uint32_t run_id = 0;          // id of the last element decoded so far (the list's head is absolute: 0 + head)
    bool prev_term = true;        // the byte before the step's first one ends a varint (the list start counts as one)
    const uint64_t p0 = b0 + 4u * lane;
    uint32_t cur = p0 < b1 ? fd_load4(value + p0) : 0u;
    for (uint64_t base = b0; base < b1; base += 4u * FD_WAVE) {
        const uint64_t p = base + 4u * lane, pn = p + 4u * FD_WAVE;
        const uint32_t nxt = pn < b1 ? fd_load4(value + pn) : 0u;      // next step's word, in flight while this one is decoded
        fd_step s;
        fd_decode_step(cur, nxt, p, b1, lane, prev_term, &s);
        const uint32_t dinc = fd_wave_scan_add(s.dsum, lane);
        f(s, run_id + dinc - s.dsum);
        run_id += __shfl(dinc, FD_WAVE - 1, FD_WAVE);
        prev_term = (__shfl(s.tb, FD_WAVE - 1, FD_WAVE) >> 3) & 1u;
        cur = nxt;
    }
}
