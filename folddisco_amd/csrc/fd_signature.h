// fd_signature.h — what the device form (k_sig.hip) and the host form (fd_signatures_host.cpp) of the index signatures share: the hash mixer and
// the pair predicate of include/fdgpu.h, stated once.  Plain C++ for a host compiler, __host__ __device__ under hipcc.
#pragma once
#include <stdint.h>
#include "../../include/fdgpu.h"

#if defined(__HIP__)            // the attributes themselves: the host files are compiled as HIP without the runtime's header
#define FD_SIG_HD __attribute__((host)) __attribute__((device)) static inline __attribute__((always_inline))
#else
#define FD_SIG_HD static inline
#endif

#define FD_SIG_EMPTY 0xffffffffu
#define FD_SIG_WORDS 70u        // u32 words of a record: n, reserved, d0, d1 (6 words), sk[64]
static_assert(sizeof(fd_signature) == 280 && sizeof(fd_sig_pair) == 12, "fd_signature / fd_sig_pair layout");

// m(h): the splitmix64 finaliser
FD_SIG_HD uint64_t fd_sig_mix(uint32_t h) {
    uint64_t z = (uint64_t)h + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
FD_SIG_HD uint32_t fd_sig_bucket(uint64_t m) { return (uint32_t)(m >> 58); }
FD_SIG_HD uint32_t fd_sig_value(uint64_t m) { return (uint32_t)(m >> 26); }

// is the pair reported?  eq = buckets whose entries agree (the ones empty in both included), E = buckets empty in both
FD_SIG_HD bool fd_sig_reported(uint32_t na, uint32_t nb, uint32_t eq, uint32_t E, uint32_t thr64) {
    const uint32_t match = eq - E, filled = 64u - E;
    return na > 0 && nb > 0 && filled > 0 && match * 64u >= thr64 * filled;
}

// is candidate x nearer than candidate y (include/fdgpu.h: signature neighbours)?  The larger match / filled, then the larger filled, then the
// smaller id: a total order.  An empty slot (match = filled = 0, id = 0xFFFFFFFF) is farther than every candidate, which has filled > 0
FD_SIG_HD bool fd_sig_nearer(uint32_t mx, uint32_t fx, uint32_t idx, uint32_t my, uint32_t fy, uint32_t idy) {
    const uint32_t l = mx * fy, r = my * fx;
    return l != r ? l > r : fx != fy ? fx > fy : idx < idy;
}
static_assert(sizeof(fd_sig_neighbor) == 8, "fd_sig_neighbor layout");
#define FD_SIG_NO_ID 0xffffffffu

// a walk order of the clusters must be a permutation of 0 .. n - 1 (fd_signatures_host.cpp; host code): -> n if it is one, the first entry that is
// not below n or repeats an earlier one if not, FD_SIG_ORDER_NOMEM when the n bits of the check could not be allocated
#define FD_SIG_ORDER_NOMEM 0xffffffffffffffffull
uint64_t fd_sig_order_fault(const uint32_t *order, uint64_t n);
