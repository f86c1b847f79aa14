// fd_postings_host.h — the part of the posting-list codec (fd_postings.h) that needs no device: the varint writer and a strict reader, and what
// the host forms of the index operations (fd_split_host.cpp, fd_rebase_host.cpp, fd_permute_host.cpp, fd_rows_host.cpp, fd_verify_host.cpp) share around them —
// the thread fan-out over slot ranges and the packaging of a result.  Plain C++, no HIP include: the host files build with a plain host compiler.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cstdlib>
#include <thread>
#include <vector>

// host writer: the varint of v at out, returns its byte length
static inline unsigned fd_put_varint(uint64_t v, uint8_t *out) {
    unsigned n = 0;
    do { uint8_t byte = v & 0x7f; v >>= 7; out[n++] = byte | (v ? 0x80 : 0); } while (v);
    return n;
}
static inline unsigned fd_varint_len_host(uint32_t v) { unsigned n = 1; while (v >>= 7) ++n; return n; }

// The varint at value[p] of a list that ends at b1: v = every payload bit of its n bytes (35 bits when the fifth byte carries more than four), and
// whether it is one.  Which statuses a caller refuses is the caller's decision: the split and the rebase take FD_VR_FIFTH_WIDE as it comes.
enum fd_vr_status {
    FD_VR_OK,
    FD_VR_FIFTH_WIDE,      // five bytes, the fifth with more than four payload bits: the value does not fit 32 bits
    FD_VR_LEAVES,          // the list ends before the varint does (n = the bytes that were there)
    FD_VR_SIXTH            // five bytes and no end: a sixth byte would follow (n = 5)
};
struct fd_varint_read { uint64_t v; unsigned n; fd_vr_status st; };
static inline fd_varint_read fd_read_varint(const uint8_t *value, uint64_t p, uint64_t b1) {
    fd_varint_read r = {0, 0, FD_VR_LEAVES};
    for (; r.n < 5 && p + r.n < b1; ++r.n) {
        const uint8_t b = value[p + r.n];
        r.v |= (uint64_t)(b & 0x7f) << (7 * r.n);
        if (!(b & 0x80)) { r.st = r.n == 4 && (b & 0x70) ? FD_VR_FIFTH_WIDE : FD_VR_OK; ++r.n; return r; }
    }
    if (r.n == 5) r.st = FD_VR_SIXTH;
    return r;
}

// threads for n slots: what the caller offers, but no thread with fewer than slots_per_thread slots
static inline uint64_t fd_host_threads(uint32_t n_threads, uint64_t n, uint64_t slots_per_thread) {
    return std::max<uint64_t>(1, std::min<uint64_t>(n_threads ? n_threads : 1, (n + slots_per_thread - 1) / slots_per_thread));
}
// f(t) for t = 0 .. T - 1, f(0) on the calling thread; thread t takes the slots n * t / T .. n * (t + 1) / T
template <class F>
static inline void fd_over_ranges(uint64_t T, F &&f) {
    std::vector<std::thread> th;
    for (uint64_t t = 1; t < T; ++t) th.emplace_back([&f, t] { f(t); });
    f(0);
    for (auto &x : th) x.join();
}

// the three malloc blocks of a result with nv value bytes and nh lists (the caller frees them with fdgpu_free); false and nothing left: out of memory
static inline bool fd_alloc_result(uint64_t nv, uint64_t nh, uint8_t **value, uint32_t **hashes, uint64_t **offsets) {
    *value = (uint8_t *)malloc(std::max<uint64_t>(nv, 1));
    *hashes = (uint32_t *)malloc(std::max<uint64_t>(nh, 1) * 4);
    *offsets = (uint64_t *)malloc((nh + 1) * 8);
    if (*value && *hashes && *offsets) return true;
    free(*value); free(*hashes); free(*offsets);
    *value = nullptr; *hashes = nullptr; *offsets = nullptr;
    return false;
}
