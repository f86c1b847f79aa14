// fd_permute_host.cpp — fdgpu_permute_host: the reorder of an index's structures (k_permute.hip) on host arrays.
// No device and no HIP call: this file also builds with a plain host compiler.  Per list: decode, map every id through new_id, std::sort, re-delta,
// re-varint.  Two passes over slot ranges, one range per thread: the new length of every list, then, behind a serial prefix sum, the bytes; both
// passes run the same routine (permute_list), once without and once with a destination.  The same checks as the device form, so the same error
// code for the same input; nothing is allocated for the result before the sizes pass has found every list sound.
#include <cstring>
#include "../../include/fdgpu.h"
#include "fd_postings_host.h"

namespace {
struct pm_in { const uint64_t *offsets; const uint8_t *value; uint64_t value_len, first_id, S; const uint32_t *new_id; };

// list k: its mapped ids in ascending order into ids (scratch), the new byte length into *len, the bytes to dst when dst is not null.
// Error bits: 1 damaged (offsets, a varint that leaves its list or is longer than five bytes, an id outside the range), 2 a list of 4 GiB
unsigned permute_list(const pm_in &A, uint64_t k, std::vector<uint32_t> &ids, uint64_t *len, uint8_t *dst) {
    const uint64_t b0 = A.offsets[k], b1 = A.offsets[k + 1];
    *len = 0;
    if (b1 <= b0 || b1 > A.value_len) return 1u;
    if (b1 - b0 > 0xffffffffull) return 2u;
    ids.clear();
    uint64_t run = 0;
    for (uint64_t q = b0; q < b1;) {
        const fd_varint_read vr = fd_read_varint(A.value, q, b1);
        if (vr.st != FD_VR_OK) return 1u;          // a sixth byte, a fifth one with more than four payload bits, or a varint that leaves the list
        run += vr.v;                               // the head is absolute: 0 + head
        if (run < A.first_id || run - A.first_id >= A.S) return 1u;
        ids.push_back((uint32_t)A.first_id + A.new_id[run - A.first_id]);
        q += vr.n;
    }
    std::sort(ids.begin(), ids.end());
    uint64_t n = 0;
    uint32_t prev = 0;
    for (size_t j = 0; j < ids.size(); ++j) {
        const uint32_t d = j ? ids[j] - prev : ids[j];
        if (dst) n += fd_put_varint(d, dst + n);
        else n += fd_varint_len_host(d);
        prev = ids[j];
    }
    if (n > 0xffffffffull) return 2u;
    *len = n;
    return 0;
}
}      // namespace

extern "C" int fdgpu_permute_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t H, const uint8_t *value, uint64_t value_len, uint64_t first_id,
                                  const uint32_t *new_id, uint64_t n, uint32_t n_threads, uint8_t **out_value, uint64_t *out_value_len,
                                  uint32_t **out_hashes, uint64_t **out_offsets) {
    if ((H && (!offsets || !hashes)) || (value_len && !value) || (n && !new_id) || !out_value || !out_value_len || !out_hashes || !out_offsets)
        return FDGPU_EINVAL;
    *out_value = nullptr; *out_hashes = nullptr; *out_offsets = nullptr; *out_value_len = 0;
    if (first_id > 0xffffffffull || first_id + n > 0xffffffffull) return FDGPU_EINVAL;
    {      // new_id must be a permutation of 0 .. n - 1
        std::vector<uint64_t> seen((n + 63) / 64, 0);
        for (uint64_t s = 0; s < n; ++s) {
            const uint64_t p = new_id[s];
            if (p >= n || (seen[p >> 6] >> (p & 63) & 1u)) return FDGPU_EINVAL;
            seen[p >> 6] |= 1ull << (p & 63);
        }
    }
    const pm_in A{offsets, value, value_len, first_id, n, new_id};
    const uint64_t T = fd_host_threads(n_threads, H, 32);
    std::vector<uint64_t> len(H);
    std::vector<unsigned> err(T, 0);
    fd_over_ranges(T, [&](uint64_t t) {
        std::vector<uint32_t> ids;
        for (uint64_t k = H * t / T; k < H * (t + 1) / T; ++k) err[t] |= permute_list(A, k, ids, &len[k], nullptr);
    });
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
    fd_over_ranges(T, [&](uint64_t t) {
        std::vector<uint32_t> ids;
        uint64_t l = 0;
        for (uint64_t k = H * t / T; k < H * (t + 1) / T; ++k) (void)permute_list(A, k, ids, &l, V + O[k]);
    });
    *out_value = V; *out_value_len = nv; *out_hashes = Hh; *out_offsets = O;
    return FDGPU_OK;
}
