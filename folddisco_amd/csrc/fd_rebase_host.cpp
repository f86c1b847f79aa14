// fd_rebase_host.cpp — fdgpu_rebase_host: the move of an index to another structure id range (k_rebase.hip) on host arrays.
// No device and no HIP call: this file also builds with a plain host compiler.  Two passes over slot ranges, one range per thread: the new length of
// every list (first varint re-encoded), then, behind a serial prefix sum, the copy.  The same checks in the same order as k_rb_sizes, so the same
// error code for the same input; nothing is allocated before the sizes pass has found every list sound.
#include <cstring>
#include "../../include/fdgpu.h"
#include "fd_postings_host.h"

namespace {
struct rb_in { const uint64_t *offsets; const uint8_t *value; uint64_t value_len, first_id, S; uint32_t shift; };

// slots [k0, k1): new lengths at len[k], new heads at head[k], bytes of the old head at nf[k]; error bits as k_rb_sizes (1: damaged, 2: 4 GiB)
unsigned size_range(const rb_in &A, uint64_t k0, uint64_t k1, uint64_t *len, uint32_t *head, uint8_t *nf) {
    unsigned err = 0;
    for (uint64_t k = k0; k < k1; ++k) {
        const uint64_t b0 = A.offsets[k], b1 = A.offsets[k + 1];
        len[k] = 0; head[k] = 0; nf[k] = 0;
        if (b1 <= b0 || b1 > A.value_len) { err |= 1u; continue; }
        const fd_varint_read vr = fd_read_varint(A.value, b0, b1);      // as fd_first_varint: five bytes at most, the low 32 bits of what they hold
        const uint32_t f = (uint32_t)vr.v;
        const unsigned n = vr.n;
        if (vr.st == FD_VR_LEAVES || vr.st == FD_VR_SIXTH || f < A.first_id || (uint64_t)f - A.first_id >= A.S) { err |= 1u; continue; }
        const uint32_t h = f + A.shift;
        const uint64_t l = b1 - b0 - n + fd_varint_len_host(h);
        if (l > 0xffffffffull) { err |= 2u; continue; }
        len[k] = l; head[k] = h; nf[k] = (uint8_t)n;
    }
    return err;
}
void copy_range(const rb_in &A, uint64_t k0, uint64_t k1, const uint64_t *out_off, const uint32_t *head, const uint8_t *nf, uint8_t *out) {
    for (uint64_t k = k0; k < k1; ++k) {
        const uint64_t b0 = A.offsets[k] + nf[k], b1 = A.offsets[k + 1];
        uint8_t *d = out + out_off[k];
        d += fd_put_varint(head[k], d);
        if (b1 > b0) memcpy(d, A.value + b0, b1 - b0);
    }
}
}      // namespace

extern "C" int fdgpu_rebase_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t H, const uint8_t *value, uint64_t value_len, uint64_t first_id,
                                 uint64_t new_first_id, uint64_t n_structures, uint32_t n_threads, uint8_t **out_value, uint64_t *out_value_len,
                                 uint32_t **out_hashes, uint64_t **out_offsets) {
    if ((H && (!offsets || !hashes)) || (value_len && !value) || !out_value || !out_value_len || !out_hashes || !out_offsets) return FDGPU_EINVAL;
    *out_value = nullptr; *out_hashes = nullptr; *out_offsets = nullptr; *out_value_len = 0;
    if (first_id > 0xffffffffull || first_id + n_structures > 0xffffffffull) return FDGPU_EINVAL;
    if (new_first_id > 0xffffffffull || new_first_id + n_structures > 0xffffffffull) return FDGPU_ERANGE;
    const rb_in A{offsets, value, value_len, first_id, n_structures, (uint32_t)(new_first_id - first_id)};
    const uint64_t T = fd_host_threads(n_threads, H, 32);
    std::vector<uint64_t> len(H);
    std::vector<uint32_t> head(H);
    std::vector<uint8_t> nf(H);
    std::vector<unsigned> err(T, 0);
    fd_over_ranges(T, [&](uint64_t t) { err[t] = size_range(A, H * t / T, H * (t + 1) / T, len.data(), head.data(), nf.data()); });
    unsigned eb = 0;
    for (unsigned e : err) eb |= e;
    if (eb & 1u) return FDGPU_EINVAL;
    if (eb & 2u) return FDGPU_ERANGE;
    uint64_t nv = 0;
    for (uint64_t k = 0; k < H; ++k) nv += len[k];
    uint8_t *V;
    uint32_t *Hh;
    uint64_t *O;
    if (!fd_alloc_result(nv, H, &V, &Hh, &O)) return FDGPU_ENOMEM;
    O[0] = 0;
    for (uint64_t k = 0; k < H; ++k) O[k + 1] = O[k] + len[k];
    if (H) memcpy(Hh, hashes, H * 4);
    fd_over_ranges(T, [&](uint64_t t) { copy_range(A, H * t / T, H * (t + 1) / T, O, head.data(), nf.data(), V); });
    *out_value = V; *out_value_len = nv; *out_hashes = Hh; *out_offsets = O;
    return FDGPU_OK;
}
