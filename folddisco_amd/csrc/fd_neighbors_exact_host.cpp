// fd_neighbors_exact_host.cpp — fdgpu_rows_neighbors_host: the exact neighbours (k_exact.hip) over host arrays.
// No device and no HIP call: this file also builds with a plain host compiler.  Threads take ranges of queries; each has one counter array
// of S and a list of the positions it touched, so a query costs its postings and not S.  A query's k-list is kept sorted under
// fd_row_nearer, a total order: the result does not depend on the order in which the structures are met, nor on the thread count.
#include <cstdlib>
#include "fd_row_neighbor.h"
#include "fd_postings_host.h"

namespace {
enum : unsigned { XN_DAMAGED = 1u, XN_LENGTHS = 2u };
struct xn_in {
    const uint32_t *q_hashes; const uint64_t *q_off;
    const uint32_t *d_hashes; const uint64_t *d_offsets; uint64_t H; const uint8_t *value; uint64_t value_len, first_id, S;
    const uint32_t *d_len, *exclude; uint32_t k, T;
};

// the ids of list t into the counters; an id outside D, a varint that is none or offsets that do not ascend inside the value bytes: damaged
unsigned count_list(const xn_in &A, uint64_t t, uint32_t *cnt, std::vector<uint32_t> &touched) {
    const uint64_t b0 = A.d_offsets[t], b1 = A.d_offsets[t + 1];
    if (b1 <= b0 || b1 > A.value_len || (A.value[b1 - 1] & 0x80)) return XN_DAMAGED;
    uint64_t run = 0;
    for (uint64_t p = b0; p < b1;) {
        const fd_varint_read vr = fd_read_varint(A.value, p, b1);
        if (vr.st != FD_VR_OK) return XN_DAMAGED;
        run += vr.v;                                   // the head is absolute: 0 + head
        if (run < A.first_id || run - A.first_id >= A.S) return XN_DAMAGED;
        const uint32_t loc = (uint32_t)(run - A.first_id);
        if (cnt[loc]++ == 0) touched.push_back(loc);
        p += vr.n;
    }
    return 0;
}

unsigned one_query(const xn_in &A, uint64_t q, uint32_t *cnt, std::vector<uint32_t> &touched, fd_row_neighbor *row) {
    const uint64_t r0 = A.q_off[q], r1 = A.q_off[q + 1];
    const uint32_t len_q = (uint32_t)(r1 - r0), skip = A.exclude ? A.exclude[q] : FD_ROW_NO_ID;
    unsigned err = 0;
    touched.clear();
    for (uint64_t i = r0; i < r1; ++i) {
        const uint32_t *at = std::lower_bound(A.d_hashes, A.d_hashes + A.H, A.q_hashes[i]);
        if (at != A.d_hashes + A.H && *at == A.q_hashes[i]) err |= count_list(A, (uint64_t)(at - A.d_hashes), cnt, touched);
    }
    uint32_t filled = 0;                               // row[0 .. filled) sorted, nearest first
    for (const uint32_t loc : touched) {
        const uint32_t inter = cnt[loc], dl = A.d_len[loc], id = (uint32_t)(A.first_id + loc);
        cnt[loc] = 0;
        if (inter > std::min(len_q, dl)) { err |= XN_LENGTHS; continue; }
        const uint32_t uni = len_q + dl - inter;
        if (id == skip || !fd_row_candidate(inter, uni, A.T)) continue;
        if (filled == A.k && !fd_row_nearer(inter, uni, id, row[filled - 1].inter, row[filled - 1].uni, row[filled - 1].id)) continue;
        uint32_t s = filled < A.k ? filled++ : filled - 1;
        for (; s > 0 && fd_row_nearer(inter, uni, id, row[s - 1].inter, row[s - 1].uni, row[s - 1].id); --s) row[s] = row[s - 1];
        row[s] = fd_row_neighbor{id, inter, uni, fd_row_flags(id, inter, uni, len_q)};
    }
    return err;
}
}      // namespace

extern "C" int fdgpu_rows_neighbors_host(const uint32_t *q_hashes, const uint64_t *q_off, uint64_t nQ, const uint32_t *d_hashes, const uint64_t *d_offsets,
                                         uint64_t n_hashes, const uint8_t *d_value, uint64_t value_len, uint64_t first_id, uint64_t S, const uint32_t *d_len,
                                         const uint32_t *exclude, uint32_t k, uint32_t floor_e4, uint32_t n_threads, fd_row_neighbor **out) {
    if (!out) return FDGPU_EINVAL;
    *out = nullptr;
    if (k < 1 || k > FD_ROW_MAX_K || floor_e4 > FD_ROW_FLOOR_MAX || (S && !d_len)) return FDGPU_EINVAL;
    if ((nQ && !q_off) || (n_hashes && (!d_hashes || !d_offsets)) || (value_len && !d_value)) return FDGPU_EINVAL;
    if (first_id > 0xffffffffull || first_id + S > 0xffffffffull || nQ > 0xffffffffull) return FDGPU_EINVAL;
    for (uint64_t q = 0; q < nQ; ++q) {
        if (q_off[q + 1] < q_off[q] || q_off[q + 1] - q_off[q] > 0xffffffffull || (q_off[q + 1] && !q_hashes)) return FDGPU_EINVAL;
        if (exclude && exclude[q] != FD_ROW_NO_ID && (exclude[q] < first_id || exclude[q] - first_id >= S)) return FDGPU_EINVAL;
    }
    const uint64_t n_rec = nQ * k;
    fd_row_neighbor *res = (fd_row_neighbor *)malloc(std::max<uint64_t>(n_rec, 1) * sizeof(fd_row_neighbor));
    if (!res) return FDGPU_ENOMEM;
    const fd_row_neighbor none = {FD_ROW_NO_ID, 0, 0, 0};
    for (uint64_t i = 0; i < std::max<uint64_t>(n_rec, 1); ++i) res[i] = none;
    const xn_in A{q_hashes, q_off, d_hashes, d_offsets, n_hashes, d_value, value_len, first_id, S, d_len, exclude, k, floor_e4};
    const uint64_t T = fd_host_threads(n_threads, nQ, 1);
    std::vector<unsigned> err(T, 0);
    std::vector<int> nomem(T, 0);
    if (S && n_hashes)
        fd_over_ranges(T, [&](uint64_t t) {
            std::vector<uint32_t> cnt, touched;
            try { cnt.assign(S, 0u); touched.reserve(S); } catch (...) { nomem[t] = 1; return; }      // at most S positions are touched: no growth later
            for (uint64_t q = nQ * t / T; q < nQ * (t + 1) / T; ++q) err[t] |= one_query(A, q, cnt.data(), touched, res + q * k);
        });
    unsigned eb = 0;
    int nm = 0;
    for (uint64_t t = 0; t < T; ++t) { eb |= err[t]; nm |= nomem[t]; }
    if (eb || nm) { free(res); return nm ? FDGPU_ENOMEM : FDGPU_EINVAL; }
    *out = res;
    return FDGPU_OK;
}
