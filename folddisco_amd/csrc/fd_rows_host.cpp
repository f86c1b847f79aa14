// fd_rows_host.cpp — fdgpu_rows_host: the rows of the transposed index (k_rows.hip) on host arrays.
// No device and no HIP call: this file also builds with a plain host compiler.  Two passes over the lists in hash order, count then place:
//   1. threads over list ranges: every list checked (the same checks as the device form, so the same error code for the same input) and its ids
//      inside the window counted; a serial prefix sum gives every list its place in the stream
//   2. threads over list ranges: the stream (id - id_lo, hash) in (hash, id) order
//   3. threads over id ranges: each reads the whole stream in order and counts, then, behind a serial prefix sum, places the elements of its own
//      rows.  A row receives its hashes in stream order, which is ascending; no two threads touch the same row, so the result does not depend on
//      the thread count.
// Nothing is allocated for the result before pass 1 has found every list sound.
#include <cstring>
#include "../../include/fdgpu.h"
#include "fd_postings_host.h"

namespace {
struct rw_in { const uint64_t *offsets; const uint8_t *value; uint64_t value_len, first_id, S, lo, hi; };

// list k: its ids inside [lo, hi) counted into *n and, when key is not null, written there less lo.  A list is ascending: one whose head is
// already at or above hi holds nothing of the window and is left after its head (the device form does not walk it either).
// Error bits: 1 damaged (offsets, a varint that leaves its list or is no u32, an id outside the range), 2 a list of 4 GiB
unsigned rows_list(const rw_in &A, uint64_t k, uint64_t *n, uint32_t *key) {
    const uint64_t b0 = A.offsets[k], b1 = A.offsets[k + 1];
    *n = 0;
    if (b1 <= b0 || b1 > A.value_len) return 1u;
    if (b1 - b0 > 0xffffffffull) return 2u;
    if (A.value[b1 - 1] & 0x80) return 1u;
    uint64_t run = 0, c = 0;
    for (uint64_t q = b0; q < b1;) {
        const fd_varint_read vr = fd_read_varint(A.value, q, b1);
        if (vr.st != FD_VR_OK) return 1u;
        run += vr.v;                               // the head is absolute: 0 + head
        if (run < A.first_id || run - A.first_id >= A.S) return 1u;
        if (q == b0 && run >= A.hi) break;
        if (run >= A.lo && run < A.hi) { if (key) key[c] = (uint32_t)(run - A.lo); ++c; }
        q += vr.n;
    }
    *n = c;
    return 0;
}
}      // namespace

extern "C" int fdgpu_rows_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t H, const uint8_t *value, uint64_t value_len, uint64_t first_id,
                               uint64_t n_structures, uint64_t id_lo, uint64_t id_hi, uint32_t n_threads, uint32_t **row_hashes, uint64_t **row_off) {
    if (!row_hashes || !row_off) return FDGPU_EINVAL;
    *row_hashes = nullptr; *row_off = nullptr;
    if ((H && (!offsets || !hashes)) || (value_len && !value)) return FDGPU_EINVAL;
    if (first_id > 0xffffffffull || first_id + n_structures > 0xffffffffull) return FDGPU_EINVAL;
    if (id_lo < first_id || id_lo > id_hi || id_hi > first_id + n_structures) return FDGPU_EINVAL;
    const uint64_t W = id_hi - id_lo;
    const rw_in A{offsets, value, value_len, first_id, n_structures, id_lo, id_hi};
    const uint64_t T = fd_host_threads(n_threads, H, 32);
    std::vector<uint64_t> base(H + 1, 0);
    if (W) {
        std::vector<unsigned> err(T, 0);
        fd_over_ranges(T, [&](uint64_t t) {
            for (uint64_t k = H * t / T; k < H * (t + 1) / T; ++k) err[t] |= rows_list(A, k, &base[k + 1], nullptr);
        });
        unsigned eb = 0;
        for (unsigned e : err) eb |= e;
        if (eb & 1u) return FDGPU_EINVAL;
        if (eb & 2u) return FDGPU_ERANGE;
        for (uint64_t k = 0; k < H; ++k) base[k + 1] += base[k];
    }
    const uint64_t n = base[H];
    if (n > 0xffffffffull) return FDGPU_ERANGE;
    uint32_t *R = (uint32_t *)malloc(std::max<uint64_t>(n, 1) * 4);
    uint64_t *O = (uint64_t *)calloc(W + 1, 8);
    if (!R || !O) { free(R); free(O); return FDGPU_ENOMEM; }
    if (n) {
        std::vector<uint32_t> key, val;
        try { key.resize(n); val.resize(n); } catch (...) { free(R); free(O); return FDGPU_ENOMEM; }
        fd_over_ranges(T, [&](uint64_t t) {
            uint64_t c = 0;
            for (uint64_t k = H * t / T; k < H * (t + 1) / T; ++k) {
                (void)rows_list(A, k, &c, key.data() + base[k]);
                std::fill(val.begin() + base[k], val.begin() + base[k + 1], hashes[k]);
            }
        });
        const uint64_t T2 = fd_host_threads(n_threads, W, 256);
        fd_over_ranges(T2, [&](uint64_t t) {           // O[s + 1] = length of row s
            const uint64_t s0 = W * t / T2, s1 = W * (t + 1) / T2;
            for (uint64_t i = 0; i < n; ++i) if (key[i] >= s0 && key[i] < s1) ++O[key[i] + 1];
        });
        for (uint64_t s = 0; s < W; ++s) O[s + 1] += O[s];
        fd_over_ranges(T2, [&](uint64_t t) {
            const uint64_t s0 = W * t / T2, s1 = W * (t + 1) / T2;
            std::vector<uint64_t> at(O + s0, O + s1);      // next free place of every row of the range
            for (uint64_t i = 0; i < n; ++i) if (key[i] >= s0 && key[i] < s1) R[at[key[i] - s0]++] = val[i];
        });
    }
    *row_hashes = R; *row_off = O;
    return FDGPU_OK;
}
