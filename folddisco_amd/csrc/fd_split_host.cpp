// fd_split_host.cpp — fdgpu_split_host: the cut of an index by structure id range (k_split.hip) on host arrays, one list after the other.
// No device and no HIP call: this file also builds with a plain host compiler.  Every thread cuts a range of slots into buffers of its own, the
// parts are the threads' buffers in slot order.
#include <cstring>
#include "../../include/fdgpu.h"
#include "fd_postings_host.h"

namespace {
struct sh_piece { std::vector<uint8_t> value; std::vector<uint32_t> hashes; std::vector<uint64_t> ends; };      // ends: value bytes after every list

// slots [k0, k1) -> out[r] for every part; false: an id outside the bounds, ids that do not ascend or a varint that leaves its list
bool cut_range(const uint32_t *hashes, const uint64_t *offsets, const uint8_t *value, uint64_t value_len, uint32_t NP, const uint64_t *bounds,
               uint64_t k0, uint64_t k1, sh_piece *out) {
    for (uint64_t k = k0; k < k1; ++k) {
        const uint64_t b0 = offsets[k], b1 = offsets[k + 1];
        if (b1 <= b0 || b1 > value_len) return false;
        uint64_t id = 0, p = b0;
        uint32_t r = 0;
        bool first = true, open = false;      // open: the list already has a piece in part r
        while (p < b1) {
            const fd_varint_read vr = fd_read_varint(value, p, b1);
            if (vr.st == FD_VR_LEAVES || vr.st == FD_VR_SIXTH) return false;      // a fifth byte is taken with every payload bit: the range test below sees the id
            const uint64_t d = vr.v, q = p + vr.n;
            if (!first && d == 0) return false;
            id += d;
            if (id < bounds[r] || id >= bounds[NP]) return false;
            bool head = first;
            while (id >= bounds[r + 1]) { ++r; head = true; open = false; }
            sh_piece &o = out[r];
            if (!open) { o.hashes.push_back(hashes[k]); o.ends.push_back(0); open = true; }
            if (head) {
                uint8_t tmp[10];
                const unsigned n = fd_put_varint(id, tmp);
                o.value.insert(o.value.end(), tmp, tmp + n);
            } else o.value.insert(o.value.end(), value + p, value + q);
            o.ends.back() = o.value.size();
            first = false;
            p = q;
        }
    }
    return true;
}
}      // namespace

extern "C" int fdgpu_split_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t H, const uint8_t *value, uint64_t value_len, uint64_t first_id,
                                uint32_t n_parts, const uint64_t *bounds, uint32_t n_threads, uint8_t **out_value, uint64_t *out_value_len,
                                uint32_t **out_hashes, uint64_t **out_offsets, uint64_t *out_n_hashes) {
    if (!offsets || (H && !hashes) || (value_len && !value) || !bounds || !out_value || !out_value_len || !out_hashes || !out_offsets || !out_n_hashes)
        return FDGPU_EINVAL;
    if (n_parts < 1 || n_parts > 64) return FDGPU_EINVAL;
    for (uint32_t r = 0; r < n_parts; ++r) { out_value[r] = nullptr; out_hashes[r] = nullptr; out_offsets[r] = nullptr; out_value_len[r] = 0; out_n_hashes[r] = 0; }
    if (bounds[0] != first_id || bounds[n_parts] > 0xffffffffull) return FDGPU_EINVAL;
    for (uint32_t r = 0; r < n_parts; ++r) if (bounds[r] > bounds[r + 1]) return FDGPU_EINVAL;
    const uint64_t T = fd_host_threads(n_threads, H, 4096);
    std::vector<std::vector<sh_piece>> got(T, std::vector<sh_piece>(n_parts));
    std::vector<char> ok(T, 1);
    fd_over_ranges(T, [&](uint64_t t) { ok[t] = cut_range(hashes, offsets, value, value_len, n_parts, bounds, H * t / T, H * (t + 1) / T, got[t].data()) ? 1 : 0; });
    for (uint64_t t = 0; t < T; ++t) if (!ok[t]) return FDGPU_EINVAL;
    for (uint32_t r = 0; r < n_parts; ++r) {
        uint64_t nh = 0, nv = 0;
        for (uint64_t t = 0; t < T; ++t) { nh += got[t][r].hashes.size(); nv += got[t][r].value.size(); }
        uint8_t *V;
        uint32_t *Hh;
        uint64_t *O;
        if (!fd_alloc_result(nv, nh, &V, &Hh, &O)) {
            for (uint32_t q = 0; q < r; ++q) { free(out_value[q]); free(out_hashes[q]); free(out_offsets[q]); out_value[q] = nullptr; out_hashes[q] = nullptr; out_offsets[q] = nullptr; }
            return FDGPU_ENOMEM;
        }
        uint64_t ph = 0, pv = 0;
        O[0] = 0;
        for (uint64_t t = 0; t < T; ++t) {
            const sh_piece &s = got[t][r];
            if (!s.value.empty()) memcpy(V + pv, s.value.data(), s.value.size());
            if (!s.hashes.empty()) memcpy(Hh + ph, s.hashes.data(), s.hashes.size() * 4);
            for (size_t k = 0; k < s.ends.size(); ++k) O[ph + k + 1] = pv + s.ends[k];
            ph += s.hashes.size(); pv += s.value.size();
        }
        out_value[r] = V; out_value_len[r] = nv; out_hashes[r] = Hh; out_offsets[r] = O; out_n_hashes[r] = nh;
    }
    return FDGPU_OK;
}
