// fd_verify.h — what "well formed" means for an index, stated once for the device checker (k_verify.hip, fdgpu_index_verify) and the host
// checker (fdgpu_verify_host).  The byte format itself is fd_postings.h.
//
// An index with H lists, value_len bytes and the ids first_id .. first_id + n_structures - 1.  A slot is a position 0 .. H of the offsets
// table; every class is reported at the slot where it does not hold.
//
//   table checks (slot k)
//   1 OFFSET_ENDS    offsets[0] == 0 (reported at slot 0) and offsets[H] == value_len (reported at slot H)
//   2 OFFSET_ORDER   offsets[k] < offsets[k + 1] <= value_len, k < H (no empty, reversed or out-of-file list)
//   3 HASH_ORDER     hashes[k] < hashes[k + 1], k + 1 < H
//
//   list checks (list k = bytes offsets[k] .. offsets[k + 1]); run only when the table is clean, because they use the offsets as addresses
//   4 LIST_END       the list's last byte has bit 7 clear (no varint runs across the end of the list)
//   5 VARINT_LONG    no byte sits behind five or more continuation bytes, and a byte behind exactly four (the fifth of its varint) is <= 0x0f:
//                    every varint has at most five bytes and a value below 2^32
//   6 VARINT_FORM    a varint of more than one byte does not end in 0x00 (the only form fd_put_varint and indextable.rs:93-99 write)
//   7 ZERO_DELTA     every varint after the first of a list is >= 1 (ids strictly ascend)
//   8 ID_RANGE       first id >= first_id and last id < min(first_id + n_structures, 2^32); the last id is the sum of the list's varints,
//                    taken as min(sum, 2^40), so a wrap cannot hide an overrun
//
// A list that shows class 4 or 5 is not decoded further (its values mean nothing): classes 6-8 are not reported for it.  Otherwise a list
// reports every class it shows.  H == 0 with value_len == 0 is well formed.  Every field of the report is a pure function of the index.
#pragma once
#include <stdint.h>
#include "../../include/fdgpu.h"

#if defined(__HIP__)      // hipcc; a plain host compiler takes fd_verify_host.cpp as well
#include <hip/hip_runtime.h>
#define FD_VF_HD __host__ __device__ __forceinline__
#else
#define FD_VF_HD static inline
#endif

#define FD_VF_BIT(c) (1u << ((c) - 1u))                       // class c in a slot's mask
#define FD_VF_STOP (FD_VF_BIT(4) | FD_VF_BIT(5))              // classes behind which a list is not decoded
#define FD_VF_DECODED (FD_VF_BIT(6) | FD_VF_BIT(7) | FD_VF_BIT(8))
#define FD_VF_SUM_CAP (1ull << 40)                            // a list's id sum saturates here (ids are below 2^32)

// where the next byte sits inside its varint: continuation bytes before it (5 = five or more), and whether those held any value bit
struct fd_vf_state { uint32_t pin, nz; };

// One byte of a list behind state s: the classes 5-7 it shows, its share of the list's id sum (*add) and whether it ends a varint (*term).
// first_varint: the byte belongs to the first varint of its list (class 7 does not apply to it).
FD_VF_HD uint32_t fd_vf_byte(fd_vf_state *s, uint32_t byte, bool first_varint, uint64_t *add, uint32_t *term) {
    const uint32_t low = byte & 0x7fu, pin = s->pin;
    uint32_t m = 0;
    if (pin >= 5u || (pin == 4u && byte > 0x0fu)) m |= FD_VF_BIT(5);
    *add = (uint64_t)low << (7u * (pin < 4u ? pin : 4u));
    const uint32_t nz = s->nz | (low ? 1u : 0u);
    if (byte & 0x80u) {
        *term = 0;
        s->pin = pin < 5u ? pin + 1u : 5u;
        s->nz = nz;
    } else {
        *term = 1;
        if (pin >= 1u && byte == 0u) m |= FD_VF_BIT(6);
        if (!nz && !first_varint) m |= FD_VF_BIT(7);
        s->pin = 0; s->nz = 0;
    }
    return m;
}
FD_VF_HD uint64_t fd_vf_sat(uint64_t v) { return v > FD_VF_SUM_CAP ? FD_VF_SUM_CAP : v; }
FD_VF_HD uint64_t fd_vf_id_limit(uint64_t first_id, uint64_t n_structures) {
    const uint64_t cap = 1ull << 32;
    return first_id >= cap || n_structures >= cap - first_id ? cap : first_id + n_structures;
}
// a list's final mask from what its bytes showed: class 4 from its last byte, class 8 from its first and last id, 6-8 dropped behind 4 / 5
FD_VF_HD uint32_t fd_vf_list_mask(uint32_t byte_classes, uint32_t last_byte, uint64_t first, uint64_t last, uint64_t first_id, uint64_t limit) {
    uint32_t m = byte_classes;
    if (last_byte & 0x80u) m |= FD_VF_BIT(4);
    if (first < first_id || last >= limit) m |= FD_VF_BIT(8);
    return (m & FD_VF_STOP) ? (m & ~FD_VF_DECODED) : m;
}

// the report from the 16 counters both checkers keep (fd_verify_host.cpp)
void fd_vf_fill_report(fd_verify_report *r, const uint64_t cnt[16], uint64_t H, bool list_stage, uint32_t first_hash, uint64_t first_offset);
