// fd_overlap_host.cpp — fdgpu_rows_intersect_host: the exact row overlaps (k_overlap.hip) on host CSR arrays.
// No device and no HIP call: this file also builds with a plain host compiler.  A plain two-pointer merge per pair; threads take ranges of
// pairs and each pair writes its own slot, so the result does not depend on the thread count.
#include <cstdlib>
#include "../../include/fdgpu.h"
#include "fd_postings_host.h"

namespace {
// |x[0 .. nx) ∩ y[0 .. ny)| of two ascending lists
uint32_t merge_count(const uint32_t *x, uint64_t nx, const uint32_t *y, uint64_t ny) {
    uint64_t i = 0, j = 0;
    uint32_t c = 0;
    while (i < nx && j < ny) {
        const uint32_t a = x[i], b = y[j];
        c += a == b;
        i += a <= b;
        j += b <= a;
    }
    return c;
}
}      // namespace

extern "C" int fdgpu_rows_intersect_host(const uint32_t *ha, const uint64_t *off_a, uint64_t n_a, const uint32_t *hb, const uint64_t *off_b, uint64_t n_b,
                                         const uint32_t *ka, const uint32_t *kb, uint64_t n_pairs, uint32_t n_threads, uint32_t **inter) {
    if (!inter) return FDGPU_EINVAL;
    *inter = nullptr;
    if (!off_b) { hb = ha; off_b = off_a; n_b = n_a; }
    if ((n_a && !off_a) || (n_pairs && (!ka || !kb)) || n_pairs > 0xffffffffull) return FDGPU_EINVAL;
    for (uint64_t k = 0; k < n_a; ++k) if (off_a[k + 1] < off_a[k] || (off_a[k + 1] && !ha)) return FDGPU_EINVAL;
    for (uint64_t k = 0; k < n_b; ++k) if (off_b[k + 1] < off_b[k] || (off_b[k + 1] && !hb)) return FDGPU_EINVAL;
    for (uint64_t p = 0; p < n_pairs; ++p) if (ka[p] >= n_a || kb[p] >= n_b) return FDGPU_EINVAL;
    uint32_t *out = (uint32_t *)malloc(std::max<uint64_t>(n_pairs, 1) * 4);
    if (!out) return FDGPU_ENOMEM;
    out[0] = 0;
    const uint64_t T = fd_host_threads(n_threads, n_pairs, 16);
    fd_over_ranges(T, [&](uint64_t t) {
        for (uint64_t p = n_pairs * t / T; p < n_pairs * (t + 1) / T; ++p) {
            const uint64_t a0 = off_a[ka[p]], a1 = off_a[ka[p] + 1], b0 = off_b[kb[p]], b1 = off_b[kb[p] + 1];
            out[p] = merge_count(ha + a0, a1 - a0, hb + b0, b1 - b0);
        }
    });
    *inter = out;
    return FDGPU_OK;
}
