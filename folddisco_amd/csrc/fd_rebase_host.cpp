// fd_rebase_host.cpp — fdgpu_rebase_host: the move of an index to another structure id range (k_rebase.hip) on host arrays.
// No device and no HIP call: this file also builds with a plain host compiler.  Two passes over slot ranges, one range per thread: the new length of
// every list (first varint re-encoded), then, behind a serial prefix sum, the copy.  The same checks in the same order as k_rb_sizes, so the same
// error code for the same input; nothing is allocated before the sizes pass has found every list sound.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "../../include/fdgpu.h"

namespace {
unsigned put_varint(uint32_t v, uint8_t *out) {
    unsigned n = 0;
    do { uint8_t byte = v & 0x7f; v >>= 7; out[n++] = byte | (v ? 0x80 : 0); } while (v);
    return n;
}
unsigned varint_len(uint32_t v) { unsigned n = 1; while (v >>= 7) ++n; return n; }

struct rb_in { const uint64_t *offsets; const uint8_t *value; uint64_t value_len, first_id, S; uint32_t shift; };

// slots [k0, k1): new lengths at len[k], new heads at head[k], bytes of the old head at nf[k]; error bits as k_rb_sizes (1: damaged, 2: 4 GiB)
unsigned size_range(const rb_in &A, uint64_t k0, uint64_t k1, uint64_t *len, uint32_t *head, uint8_t *nf) {
    unsigned err = 0;
    for (uint64_t k = k0; k < k1; ++k) {
        const uint64_t b0 = A.offsets[k], b1 = A.offsets[k + 1];
        len[k] = 0; head[k] = 0; nf[k] = 0;
        if (b1 <= b0 || b1 > A.value_len) { err |= 1u; continue; }
        uint32_t f = 0;
        unsigned n = 0;
        const uint64_t lim = std::min<uint64_t>(5, b1 - b0);
        for (uint64_t q = 0; q < lim; ++q) {
            f |= (uint32_t)((uint64_t)(A.value[b0 + q] & 0x7f) << (7 * q));
            if (!(A.value[b0 + q] & 0x80)) { n = (unsigned)q + 1; break; }
        }
        if (!n || f < A.first_id || (uint64_t)f - A.first_id >= A.S) { err |= 1u; continue; }
        const uint32_t h = f + A.shift;
        const uint64_t l = b1 - b0 - n + varint_len(h);
        if (l > 0xffffffffull) { err |= 2u; continue; }
        len[k] = l; head[k] = h; nf[k] = (uint8_t)n;
    }
    return err;
}
void copy_range(const rb_in &A, uint64_t k0, uint64_t k1, const uint64_t *out_off, const uint32_t *head, const uint8_t *nf, uint8_t *out) {
    for (uint64_t k = k0; k < k1; ++k) {
        const uint64_t b0 = A.offsets[k] + nf[k], b1 = A.offsets[k + 1];
        uint8_t *d = out + out_off[k];
        d += put_varint(head[k], d);
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
    const uint64_t T = std::max<uint64_t>(1, std::min<uint64_t>(n_threads ? n_threads : 1, (H + 31) / 32));      // at least 32 slots per thread
    std::vector<uint64_t> len(H);
    std::vector<uint32_t> head(H);
    std::vector<uint8_t> nf(H);
    auto over_ranges = [&](auto &&f) {
        std::vector<std::thread> th;
        for (uint64_t t = 1; t < T; ++t) th.emplace_back(f, t);
        f(0);
        for (auto &x : th) x.join();
    };
    std::vector<unsigned> err(T, 0);
    over_ranges([&](uint64_t t) { err[t] = size_range(A, H * t / T, H * (t + 1) / T, len.data(), head.data(), nf.data()); });
    unsigned eb = 0;
    for (unsigned e : err) eb |= e;
    if (eb & 1u) return FDGPU_EINVAL;
    if (eb & 2u) return FDGPU_ERANGE;
    uint64_t *O = (uint64_t *)malloc((H + 1) * 8);
    uint32_t *Hh = (uint32_t *)malloc(std::max<uint64_t>(H, 1) * 4);
    if (!O || !Hh) { free(O); free(Hh); return FDGPU_ENOMEM; }
    uint64_t nv = 0;
    for (uint64_t k = 0; k < H; ++k) { O[k] = nv; nv += len[k]; }
    O[H] = nv;
    uint8_t *V = (uint8_t *)malloc(std::max<uint64_t>(nv, 1));
    if (!V) { free(O); free(Hh); return FDGPU_ENOMEM; }
    if (H) memcpy(Hh, hashes, H * 4);
    over_ranges([&](uint64_t t) { copy_range(A, H * t / T, H * (t + 1) / T, O, head.data(), nf.data(), V); });
    *out_value = V; *out_value_len = nv; *out_hashes = Hh; *out_offsets = O;
    return FDGPU_OK;
}
