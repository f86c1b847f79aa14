// fd_row_neighbor.h — what the device form (k_exact.hip) and the host form (fd_neighbors_exact_host.cpp) of the exact neighbours share: the
// candidate predicate, the order and the record's flag of include/fdgpu.h, stated once.  Plain C++ for a host compiler, __host__ __device__
// under hipcc.
#pragma once
#include <stdint.h>
#include "../../include/fdgpu.h"

#if defined(__HIP__)            // the attributes themselves: the host files are compiled as HIP without the runtime's header
#define FD_ROW_HD __attribute__((host)) __attribute__((device)) static inline __attribute__((always_inline))
#else
#define FD_ROW_HD static inline
#endif

static_assert(sizeof(fd_row_neighbor) == 16, "fd_row_neighbor layout");
#define FD_ROW_NO_ID 0xffffffffu
#define FD_ROW_MAX_K 32u
#define FD_ROW_FLOOR_MAX 10000u

// does a structure with inter shared hashes and a union of uni reach the floor T (floor_e4)?  The expression of indexio.jaccard_reaches;
// T = 0: any shared hash.  inter > 0 implies uni > 0
FD_ROW_HD bool fd_row_candidate(uint32_t inter, uint32_t uni, uint32_t T) {
    return inter > 0 && (uint64_t)inter * 10000ull >= (uint64_t)T * uni;
}

// is candidate x nearer than candidate y?  The larger inter / uni by cross products, then the larger inter, then the smaller id: a total order.
// An empty slot (inter = uni = 0, id = 0xFFFFFFFF) is farther than every candidate, which has inter > 0
FD_ROW_HD bool fd_row_nearer(uint32_t ix, uint32_t ux, uint32_t idx, uint32_t iy, uint32_t uy, uint32_t idy) {
    const uint64_t l = (uint64_t)ix * uy, r = (uint64_t)iy * ux;
    return l != r ? l > r : ix != iy ? ix > iy : idx < idy;
}

// the flags of a record of a query row of len_q hashes: FD_ROW_EQUAL when inter == |R_q| == d_len, which uni == inter says of d_len
FD_ROW_HD uint32_t fd_row_flags(uint32_t id, uint32_t inter, uint32_t uni, uint32_t len_q) {
    return id != FD_ROW_NO_ID && inter == len_q && uni == inter ? FD_ROW_EQUAL : 0u;
}
