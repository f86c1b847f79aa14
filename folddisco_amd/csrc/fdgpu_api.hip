// fdgpu_api.hip — C ABI of libfdgpu.so (include/fdgpu.h): the context, the result pool, batches, the hash constants, the index object (the other half of S2:
// fd_index_new, destroy, accessors), export / load / save and the pinned copy paths.  The hashers and the build are in fd_api_build.hip, S3 in
// fd_api_count.hip, S4 in fd_api_match.hip.  No CPU fallback exists: every entry point fails with FDGPU_EHIP if no gfx950 device answers.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <sys/mman.h>
#include <atomic>
#include <thread>
#include "fdgpu_internal.h"
#include <fcntl.h>
#include <unistd.h>
#include <cerrno>
#include <cstring>

#include "fd_api_common.h"
#include "fd_postings.h"

// ---- small kernels used only here ------------------------------------------------------------------
__global__ void k_uniq_flags(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ ids, uint64_t n, uint8_t *__restrict__ flags) {
    uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) flags[p] = (p == 0 || keys[p] != keys[p - 1] || ids[p] != ids[p - 1]) ? 1 : 0;
}
__global__ void k_compact(const uint32_t *__restrict__ keys, const uint8_t *__restrict__ flags, const uint64_t *__restrict__ pos, uint64_t n,
                          uint32_t *__restrict__ out) {
    uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n && flags[p]) out[pos[p]] = keys[p];
}
__global__ void k_gather_u64(const uint64_t *__restrict__ src, const uint64_t *__restrict__ idx, uint64_t n, uint64_t *__restrict__ dst) {
    uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) dst[p] = src[idx[p]];
}
void fd_launch_uniq_flags(const uint32_t *keys, const uint32_t *ids, uint64_t n, uint8_t *flags, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_uniq_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, ids, n, flags);
}
void fd_launch_compact(const uint32_t *keys, const uint8_t *flags, const uint64_t *pos, uint64_t n, uint32_t *out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_compact, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, flags, pos, n, out);
}
void fd_launch_gather_u64(const uint64_t *src, const uint64_t *idx, uint64_t n, uint64_t *dst, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_gather_u64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, idx, n, dst);
}

// postings of an index = varint terminators of its value bytes (bytes without the continuation bit)
__global__ __launch_bounds__(256) void k_count_postings(const uint8_t *__restrict__ value, uint64_t n, unsigned long long *__restrict__ out) {
    unsigned long long acc = 0;
    for (uint64_t p = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16; p < n; p += (uint64_t)gridDim.x * 256 * 16)
        for (uint64_t k = p; k < n && k < p + 16; ++k) acc += !(value[k] & 0x80u);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}
hipError_t fd_count_postings(fdgpu_ctx *c, const uint8_t *value, uint64_t n, uint64_t *out) {
    unsigned long long np = 0;
    hipError_t e = hipSuccess;
    if (n) {
        e = c->ws[WS_TOTAL].ensure(64);
        if (e == hipSuccess) e = hipMemsetAsync(c->ws[WS_TOTAL].p, 0, 8, c->stream);
        if (e == hipSuccess) { hipLaunchKernelGGL(k_count_postings, dim3(2048), dim3(256), 0, c->stream, value, n, c->ws[WS_TOTAL].as<unsigned long long>()); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipMemcpyAsync(&np, c->ws[WS_TOTAL].p, 8, hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    *out = np;
    return e;
}

// ---- context ------------------------------------------------------------------------------------------------
extern "C" const char *fdgpu_version(void) { return "folddisco_amd 0.1 (gfx950)"; }

// Start-up self-check (FDGPU_SELFCHECK=0 skips it):
//  1. device known-answer test: the six 4CHA triad hashes of the reference's own test (controller/graph.rs:71-79) through the
//     generic, table and speculative evaluations (k_selfcheck) — a mismatch fails fdgpu_create;
//  2. host libm probe: the device restates glibc 2.35's sinf / cosf / acosf / atan2f bit for bit (fd_libm.h).  A reference (Rust)
//     build on a host whose libm rounds differently (e.g. glibc >= 2.40 CORE-MATH) would hash differently from this library, so the
//     same restatement compiled for the host is compared with the host's libm around every quantiser threshold; the verdict is
//     kept in the context (fdgpu_host_libm_matches) and a mismatch is reported once on stderr.
static int fd_selfcheck(fdgpu_ctx *c) {
    const char *e = getenv("FDGPU_SELFCHECK");
    if (e && e[0] == '0') return FDGPU_OK;
    fd_hash_params p;
    memset(&p, 0, sizeof p);
    p.dist_cutoff = 20.0f; p.hash_type = FDGPU_HASH_PDBTR;
    const fd_hash_consts C = make_consts(&p);
    uint32_t *d = nullptr, h[24];
    HIPCHK(c, hipMalloc((void **)&d, sizeof h));
    fd_launch_selfcheck(C.q, d, c->stream);
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (he != hipSuccess) { c->err = std::string("self-check launch: ") + hipGetErrorString(he); return FDGPU_EHIP; }
    static const uint32_t want[6] = {109329223u, 116878724u, 271858548u, 284511716u, 506948936u, 512052558u};
    for (int k = 0; k < 24; ++k)
        if (h[k] != want[k % 6]) {
            char b[256];
            snprintf(b, sizeof b, "self-check failed: 4CHA triad hash %d (%s evaluation) is %u, the reference's literal is %u (controller/graph.rs:71-79)", k % 6,
                     k < 6 ? "generic" : k < 12 ? "table" : k < 18 ? "speculative" : "speculative + squared-distance table", h[k], want[k % 6]);
            c->err = b;
            return FDGPU_EHIP;
        }
    // host libm generation: the restatement (fd_libm.h, compiled for the host here) against libm around the thresholds the quantiser uses
    int ok = 1;
    auto same = [](float a, float b) { uint32_t x, y; memcpy(&x, &a, 4); memcpy(&y, &b, 4); return x == y || (a != a && b != b); };
    for (int k = 1; k < FD_THETA_NSEG && ok; ++k) {
        float t;
        memcpy(&t, &fd_theta_thr_bits[k], 4);
        for (int u = -64; u <= 64 && ok; ++u) {
            uint32_t bits = fd_theta_thr_bits[k] + (uint32_t)u;
            float x;
            memcpy(&x, &bits, 4);
            if (!(x >= -1.0f && x <= 1.0f)) continue;
            const float a = acosf(x);
            ok = same(fd_acosf(x), a) && same(fd_sinf(a), sinf(a)) && same(fd_cosf(a), cosf(a));
        }
    }
    for (int m = 0; m < 4 && ok; ++m)
        for (int k = 1; k < FD_TOR_MAXSEG && ok; ++k)
            for (int u = -64; u <= 64 && ok; ++u) {
                uint32_t bits = fd_tor_thr_bits[m][k] + (uint32_t)u;
                float r;
                memcpy(&r, &bits, 4);
                if (!(r == r) || r > 3.0e38f) continue;
                const float y = (m & 1) ? -r : r, x = (m & 2) ? -1.0f : 1.0f;
                const float a = -atan2f(y, x);
                ok = same(-fd_atan2f(y, x), a) && same(fd_sinf(a), sinf(a)) && same(fd_cosf(a), cosf(a));
            }
    c->host_libm_matches = ok;
    if (!ok) {
        static bool warned = false;
        if (!warned) {
            warned = true;
            fprintf(stderr, "[fdgpu] warning: this host's libm (sinf/cosf/acosf/atan2f) differs from the glibc 2.35 generation the device arithmetic restates; a "
                            "reference build on this host can hash residue pairs at bin edges differently (rerun tools/gen_bin_tables.c + tools/check_libm.c)\n");
        }
    }
    return FDGPU_OK;
}
// 1 = the host's libm agrees with the restated generation, 0 = it does not, -1 = the self-check was skipped
extern "C" int fdgpu_host_libm_matches(const fdgpu_ctx *c) { return c ? c->host_libm_matches : -1; }

static std::atomic<int> fd_live_contexts{0};      // contexts with a device + stream: the last fdgpu_destroy trims the result pool
extern "C" void fdgpu_trim(void);
extern "C" int fdgpu_create(int device, fdgpu_ctx **out) {
    if (!out) return FDGPU_EINVAL;
    *out = nullptr;
    fdgpu_ctx *c = new (std::nothrow) fdgpu_ctx();
    if (!c) return FDGPU_ENOMEM;
    c->device = device;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0 || device < 0 || device >= n) {
        // keep the context so that the caller can read the message, but report failure
        c->err = e != hipSuccess ? std::string("hipGetDeviceCount: ") + hipGetErrorString(e) : "no such HIP device";
        *out = c;
        return FDGPU_EHIP;
    }
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreate(&c->stream)) != hipSuccess) {
        c->err = std::string("hipSetDevice/hipStreamCreate: ") + hipGetErrorString(e);
        *out = c;
        return FDGPU_EHIP;
    }
    c->own_stream = true;
    c->counted = true;
    fd_live_contexts.fetch_add(1);
    if (hipMalloc((void **)&c->spec_miss, 8) == hipSuccess) (void)hipMemset(c->spec_miss, 0, 8);
    else c->spec_miss = nullptr;
    *out = c;
    return fd_selfcheck(c);
}
// number of residue pairs the speculative torsion evaluation handed to the exact routine since the last call (profiling hook)
extern "C" int fdgpu_spec_fallbacks(fdgpu_ctx *c, uint64_t *out) { FD_LOCK(c);
    if (!c || !out) return FDGPU_EINVAL;
    *out = 0;
    if (!c->spec_miss) return FDGPU_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->spec_miss, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->spec_miss, 0, 8));
    return FDGPU_OK;
}
extern "C" void fdgpu_destroy(fdgpu_ctx *c) {
    if (!c) return;
    fd_lanes_destroy(c);      // query lanes (fd_lanes.hip): queued batches run to their end, worker threads joined, sibling contexts destroyed
    if (c->spec_miss) (void)hipFree(c->spec_miss);
    for (auto &b : c->ws) b.release();
    for (auto &b : c->pool) (void)hipFree(b.p);
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    for (int k = 0; k < 16; ++k) { if (c->pin[k]) (void)hipHostFree(c->pin[k]); if (c->pin_ev[k]) (void)hipEventDestroy(c->pin_ev[k]); }
    for (int k = 0; k < FD_HP_SLOTS; ++k) if (c->hbuf[k]) (void)hipHostFree(c->hbuf[k]);
    if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    const bool last = c->counted && fd_live_contexts.fetch_sub(1) == 1;
    delete c;
    if (last) fdgpu_trim();      // the process's last context: hand the pooled (page-locked) result blocks back
}
// Returns the context's workspaces (the sort buffers of the largest build so far, query scratch) and the cached blocks of destroyed indices to
// the device.  Indices, batches and query maps stay valid; the next call allocates what it needs again.
extern "C" int fdgpu_release_workspaces(fdgpu_ctx *c) { FD_LOCK(c);
    if (!c) return FDGPU_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto &b : c->ws) b.release();
    c->pair_masks_crowded = false;
    c->pool_drop();
    (void)hipGetLastError();
    return FDGPU_OK;
}
extern "C" int fdgpu_set_stream(fdgpu_ctx *c, void *s) { FD_LOCK(c);
    if (!c) return FDGPU_EINVAL;
    if (c->own_stream && c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); c->own_stream = false; }
    if (s) { c->stream = (hipStream_t)s; return FDGPU_OK; }
    HIPCHK(c, hipStreamCreate(&c->stream));
    c->own_stream = true;
    return FDGPU_OK;
}
extern "C" int fdgpu_synchronize(fdgpu_ctx *c) { FD_LOCK(c);
    if (!c) return FDGPU_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FDGPU_OK;
}
extern "C" const char *fdgpu_last_error(const fdgpu_ctx *c) { return c ? c->err.c_str() : "null context"; }
// Result arrays of the hot query entry points (match records, residue lists, count records: megabytes per batch) come from a small
// recycling pool: a fresh malloc of that size is an mmap whose pages fault in one by one when the library fills them (1.5 of the 2.3 ms the
// record assembly of a 512-query batch took) and an munmap when the caller frees them.  Blocks are plain malloc memory; fdgpu_free puts a
// pooled block back (at most FD_OUT_POOL_BYTES are kept, the rest is freed), anything else goes to free().  Thread-safe.
#include <mutex>
#include <unordered_map>
namespace {
struct fd_out_blk { size_t cap; bool pinned; };
struct fd_out_pool {
    std::mutex mu;
    std::unordered_map<void *, fd_out_blk> live;             // blocks handed out
    std::vector<std::pair<fd_out_blk, void *>> idle;         // blocks waiting for reuse
    size_t idle_bytes = 0;
};
fd_out_pool &out_pool() { static fd_out_pool *p = new fd_out_pool(); return *p; }     // never destroyed: callers may free after static destructors ran
const size_t FD_OUT_POOL_MIN = (size_t)64 << 10;
size_t fd_out_pool_cap() {      // idle bytes kept for reuse: 256 MB, FDGPU_OUT_POOL_MB overrides (0: nothing is kept)
    static const size_t cap = [] { const char *e = getenv("FDGPU_OUT_POOL_MB"); return e ? (size_t)std::max(0L, atol(e)) << 20 : (size_t)256 << 20; }();
    return cap;
}
}
// Releases the idle blocks of the result pool (page-locked ones included).  Long-lived hosts with varying batch sizes call it when a burst
// is over; the last fdgpu_destroy of a process calls it too.  Blocks the caller still holds are untouched.
extern "C" void fdgpu_trim(void) {
    fd_out_pool &P = out_pool();
    std::vector<std::pair<fd_out_blk, void *>> drop;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        drop.swap(P.idle);
        P.idle_bytes = 0;
    }
    for (auto &b : drop) { if (b.first.pinned) (void)hipHostFree(b.second); else free(b.second); }
}
// pinned: page-locked host memory (hipHostMalloc) — the device copies its results straight into the caller's array
void *fd_out_alloc(size_t bytes, bool pinned) {
    if (bytes < FD_OUT_POOL_MIN) return malloc(bytes ? bytes : 1);
    fd_out_pool &P = out_pool();
    {
        std::lock_guard<std::mutex> lk(P.mu);
        size_t best = (size_t)-1;
        for (size_t k = 0; k < P.idle.size(); ++k)
            if (P.idle[k].first.pinned == pinned && P.idle[k].first.cap >= bytes && P.idle[k].first.cap <= 2 * bytes + (1u << 20) &&
                (best == (size_t)-1 || P.idle[k].first.cap < P.idle[best].first.cap)) best = k;
        if (best != (size_t)-1) {
            void *p = P.idle[best].second;
            const fd_out_blk b = P.idle[best].first;
            P.idle.erase(P.idle.begin() + best);
            P.idle_bytes -= b.cap;
            P.live[p] = b;
            return p;
        }
    }
    const size_t cap = bytes + bytes / 4;
    void *p = nullptr;
    bool got_pinned = false;
    if (pinned && hipHostMalloc(&p, cap, hipHostMallocPortable) == hipSuccess && p) got_pinned = true;
    else { (void)hipGetLastError(); p = malloc(cap); }
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(P.mu);
    P.live[p] = fd_out_blk{cap, got_pinned};
    return p;
}
extern "C" void fdgpu_free(void *p) {
    if (!p) return;
    fd_out_pool &P = out_pool();
    fd_out_blk b;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        auto it = P.live.find(p);
        if (it == P.live.end()) { free(p); return; }
        b = it->second;
        P.live.erase(it);
        if (P.idle_bytes + b.cap <= fd_out_pool_cap()) { P.idle.emplace_back(b, p); P.idle_bytes += b.cap; return; }
    }
    if (b.pinned) (void)hipHostFree(p); else free(p);
}
extern "C" int fdgpu_enable_timing(fdgpu_ctx *c, int on) { FD_LOCK(c); if (!c) return FDGPU_EINVAL; c->timing = on != 0; return FDGPU_OK; }
extern "C" int fdgpu_last_timings(const fdgpu_ctx *c, const char **names, float *ms, uint64_t *bytes, int cap) { FD_LOCK(c);
    if (!c) return FDGPU_EINVAL;
    int n = 0;
    for (auto &t : c->timings) {
        if (n >= cap) break;
        float m = 0.f;
        if (hipEventElapsedTime(&m, t.ev0, t.ev1) != hipSuccess) m = -1.f;
        if (names) names[n] = t.name;
        if (ms) ms[n] = m;
        if (bytes) bytes[n] = t.bytes;
        ++n;
    }
    return n;
}

// ---- batches ---------------------------------------------------------------------------------------------------
int fd_build_work_items(fdgpu_ctx *c, fdgpu_batch *b, bool with_hash_ok) {
    // one work item per (structure, 64-residue i-tile)
    std::vector<uint32_t> ws, wi;
    std::vector<uint64_t> wc;      // first column of every work item in the MSD build's mask table, + the total (fd_pair_mask_cols.h)
    std::vector<uint32_t> ro(b->n_struct + 1);
    for (uint64_t s = 0; s <= b->n_struct; ++s) ro[s] = (uint32_t)b->h_res_off[s];
    for (uint64_t s = 0; s < b->n_struct; ++s) {
        uint64_t R = b->h_res_off[s + 1] - b->h_res_off[s];
        if (R > 65535) FAIL(c, FDGPU_ERANGE, "structure with more than 65535 residues (reference max_residue, controller/mod.rs:40)");
        for (uint64_t t = 0; t < R; t += FD_WAVE) { ws.push_back((uint32_t)s); wi.push_back((uint32_t)(b->h_res_off[s] + t)); }
    }
    if (ws.size() > 0xfffffff0ull) FAIL(c, FDGPU_ERANGE, "too many tiles in one batch");
    b->n_work = (uint32_t)ws.size();
    wc.resize(ws.size() + 1);
    b->n_mask_cols = fd_mask_col_offsets(b->h_res_off.data(), b->n_struct, wc.data());
    HIPCHK(c, hipMalloc((void **)&b->res_off, ro.size() * 4));
    HIPCHK(c, hipMalloc((void **)&b->wi_col, wc.size() * 8));
    HIPCHK(c, hipMemcpyAsync(b->wi_col, wc.data(), wc.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMalloc((void **)&b->wi_struct, std::max<size_t>(ws.size(), 1) * 4));
    HIPCHK(c, hipMalloc((void **)&b->wi_i0, std::max<size_t>(wi.size(), 1) * 4));
    HIPCHK(c, hipMemcpyAsync(b->res_off, ro.data(), ro.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!ws.empty()) {
        HIPCHK(c, hipMemcpyAsync(b->wi_struct, ws.data(), ws.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(b->wi_i0, wi.data(), wi.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMalloc((void **)&b->hash_ok, std::max<uint64_t>(b->n_res, 1)));
    if (with_hash_ok) fd_launch_hash_ok(b->aa, b->cb_valid, b->hash_ok, b->n_res, c->stream);      // (a batch whose arrays are still to be filled: the caller launches it afterwards, k_batch.hip)
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));  // host vectors go out of scope
    return FDGPU_OK;
}

extern "C" int fdgpu_batch_upload(fdgpu_ctx *c, const fd_batch_desc *h, fdgpu_batch **out) { FD_LOCK(c);
    if (!c || !h || !out || !h->res_off || (h->n_struct && (!h->n_xyz || !h->ca_xyz || !h->cb_xyz || !h->aa))) return FDGPU_EINVAL;
    *out = nullptr;
    if (h->n_struct >= 0xffffffffull) FAIL(c, FDGPU_ERANGE, "too many structures in one batch");
    uint64_t R = h->res_off[h->n_struct];
    if (R >= 0xffffffffull) FAIL(c, FDGPU_ERANGE, "more than 2^32 residues in one batch");
    fdgpu_batch *b = new (std::nothrow) fdgpu_batch();
    if (!b) return FDGPU_ENOMEM;
    b->ctx = c; b->owns = true; b->n_struct = h->n_struct; b->n_res = R;
    b->h_res_off.assign(h->res_off, h->res_off + h->n_struct + 1);
    size_t rb = std::max<uint64_t>(R, 1);
    int rc = FDGPU_OK;
    auto up = [&](void **d, const void *src, size_t bytes) -> int {
        HIPCHK(c, hipMalloc(d, std::max<size_t>(bytes, 4)));
        if (bytes) HIPCHK(c, hipMemcpyAsync(*d, src, bytes, hipMemcpyHostToDevice, c->stream));
        return FDGPU_OK;
    };
    if ((rc = up((void **)&b->n_xyz, h->n_xyz, R * 12)) || (rc = up((void **)&b->ca_xyz, h->ca_xyz, R * 12)) ||
        (rc = up((void **)&b->cb_xyz, h->cb_xyz, R * 12)) || (rc = up((void **)&b->aa, h->aa, R))) { fdgpu_batch_destroy(b); return rc; }
    if (h->cb_valid && (rc = up((void **)&b->cb_valid, h->cb_valid, R))) { fdgpu_batch_destroy(b); return rc; }
    (void)rb;
    if ((rc = fd_build_work_items(c, b))) { fdgpu_batch_destroy(b); return rc; }
    *out = b;
    return FDGPU_OK;
}

extern "C" int fdgpu_batch_wrap_device(fdgpu_ctx *c, const fd_batch_desc *d, uint64_t total_residues, fdgpu_batch **out) { FD_LOCK(c);
    if (!c || !d || !out || !d->res_off) return FDGPU_EINVAL;
    *out = nullptr;
    fdgpu_batch *b = new (std::nothrow) fdgpu_batch();
    if (!b) return FDGPU_ENOMEM;
    b->ctx = c; b->owns = false; b->n_struct = d->n_struct; b->n_res = total_residues;
    b->n_xyz = (float *)d->n_xyz; b->ca_xyz = (float *)d->ca_xyz; b->cb_xyz = (float *)d->cb_xyz;
    b->aa = (uint8_t *)d->aa; b->cb_valid = (uint8_t *)d->cb_valid;
    b->h_res_off.resize(d->n_struct + 1);
    hipError_t e = hipMemcpy(b->h_res_off.data(), d->res_off, (d->n_struct + 1) * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { c->err = std::string("wrap_device: ") + hipGetErrorString(e); delete b; return FDGPU_EHIP; }
    if (b->h_res_off[d->n_struct] != total_residues) { c->err = "wrap_device: res_off[n] != total_residues"; delete b; return FDGPU_EINVAL; }
    int rc = fd_build_work_items(c, b);
    if (rc) { fdgpu_batch_destroy(b); return rc; }
    *out = b;
    return FDGPU_OK;
}

extern "C" void fdgpu_batch_destroy(fdgpu_batch *b) {
    if (!b) return;
    if (b->owns) { (void)hipFree(b->n_xyz); (void)hipFree(b->ca_xyz); (void)hipFree(b->cb_xyz); (void)hipFree(b->aa); (void)hipFree(b->cb_valid); }
    (void)hipFree(b->hash_ok); (void)hipFree(b->res_off); (void)hipFree(b->wi_struct); (void)hipFree(b->wi_i0);
    (void)hipFree(b->wi_col);
    delete b;
}
extern "C" uint64_t fdgpu_batch_num_structures(const fdgpu_batch *b) { return b ? b->n_struct : 0; }
extern "C" uint64_t fdgpu_batch_num_residues(const fdgpu_batch *b) { return b ? b->n_res : 0; }

// ---- hash constants ------------------------------------------------------------------------------------------------
// per-encoding bin rules: {cap_dist, default_dist, cap_angle, default_angle} (perfect_hash of pdb_motif.rs:27-40,
// pdb_motif_sincos.rs:19-31, pdb_tr.rs:22-35, folddisco_angle.rs:26-40, folddisco_dist.rs:23-37)
bool fd_hash_type_supported(uint32_t t) { return t <= 8u; }   // HashType::get_with_index 0..8 (geometry/core.rs:26-40)
// nbd / nba: requested bin counts.  either_zero_defaults: the rule of the single-configuration callers (either count 0 -> both
// defaults, controller/feature.rs:216-223, query.rs:72-77); the per-encoding perfect_hash itself treats the two counts
// independently (pdb_tr.rs:22-35 etc.), which is what the --multiple-bins list reaches (zero counts are rejected there).
fd_hash_consts make_consts_bins(const fd_hash_params *p, uint32_t nbd_req, uint32_t nba_req, bool either_zero_defaults) {
    // convert.rs:32-36 quantiser factors evaluated in f32 exactly like the reference
    const uint32_t type = p->hash_type;
    uint32_t cap_d = 16, def_d = 16, cap_a = 4, def_a = 4;
    if (type == FD_HASH_PDBMOTIF) { cap_d = 32; def_d = 18; cap_a = 32; def_a = 9; }
    else if (type == FD_HASH_PDBMOTIF_SINCOS) { cap_d = 16; def_d = 8; cap_a = 16; def_a = 3; }
    else if (type == FD_HASH_FD_ANGLE) { cap_d = 8; def_d = 8; cap_a = 32; def_a = 32; }
    else if (type == FD_HASH_FD_DIST) { cap_d = 32; def_d = 32; cap_a = 16; def_a = 16; }
    else if (type == FD_HASH_TRROSETTA) { cap_d = 8; def_d = 8; cap_a = 4; def_a = 3; }        // trrosetta.rs:62-64, convert.rs NBIN_DIST / NBIN_SIN_COS
    else if (type == FD_HASH_PPF || type == FD_HASH_TERTIARY) { cap_d = 16; def_d = 8; cap_a = 8; def_a = 3; }   // ppf.rs:16-31, tertiary_interaction.rs:23-36
    else if (type == FD_HASH_HYBRID) { cap_d = 16; def_d = 16; cap_a = 4; def_a = 4; }         // hybrid.rs:22-35
    // either bin count 0 -> perfect_hash_default (controller/feature.rs:216-223, query.rs:72-77)
    const bool dflt = either_zero_defaults && (nbd_req == 0 || nba_req == 0);
    float nd = (dflt || nbd_req == 0) ? (float)def_d : (nbd_req > cap_d ? (float)cap_d : (float)nbd_req);
    float na = (dflt || nba_req == 0) ? (float)def_a : (nba_req > cap_a ? (float)cap_a : (float)nba_req);
    fd_hash_consts C;
    C.seg_mul = 1; C.seg_cfg = 0;
    const float PI_F = 3.14159274f;
    float a_min = -1.0f, a_max = 1.0f;                                         // sin / cos fields
    if (type == FD_HASH_PDBMOTIF) { a_min = 0.0f; a_max = 180.0f; }            // degrees
    else if (type == FD_HASH_FD_ANGLE || type == FD_HASH_FD_DIST) { a_min = -PI_F; a_max = PI_F; }
    volatile float cont_d = (20.0f - 2.0f) / (nd - 1.0f);
    volatile float cont_a = (a_max - a_min) / (na - 1.0f);
    float n180 = type == FD_HASH_FD_ANGLE ? fminf(na, 32.0f) : fminf(na, 8.0f);
    volatile float cont_t = (PI_F - 0.0f) / (n180 - 1.0f);
    C.q.dist_disc = 1.0f / cont_d;
    C.q.ang_disc = 1.0f / cont_a;
    C.q.ang2_disc = 1.0f / cont_t;
    C.q.type = type;
    // largest f32 d2 with sqrtf(d2) <= cutoff (sqrtf is correctly rounded on host and device)
    float cut = p->dist_cutoff;
    float d2 = cut * cut;
    while (sqrtf(d2) > cut) d2 = nextafterf(d2, 0.0f);
    while (sqrtf(nextafterf(d2, INFINITY)) <= cut) d2 = nextafterf(d2, INFINITY);
    C.d2_max = d2;
    // default angle bins: table form; the index build evaluates the torsion fields speculatively with an exact fallback
    // (fd_geom.h fd_pair_both_spec) unless FDGPU_EXACT=1
    const char *ex = getenv("FDGPU_EXACT");   // read per call: tests flip it inside one process
    const bool exact_only = ex && ex[0] == '1';
    C.use_tab = (type == FD_HASH_PDBTR && na == 4.0f) ? (exact_only ? 1 : 2) : 0;
    // default 16 distance bins as well: the MSD build's pair kernel takes the two distance fields from the exhaustive squared-distance table
    // (fd_dist_table.h; FDGPU_DTAB=0 keeps sqrt + quantiser, for measurements and the tests that compare the two)
    const char *dt = getenv("FDGPU_DTAB");
    if (C.use_tab == 2 && nd == 16.0f && !(dt && dt[0] == '0')) C.use_tab = 3;
    C.spec_miss = nullptr;
    return C;
}

fd_hash_consts make_consts(const fd_hash_params *p) { return make_consts_bins(p, p->nbin_dist, p->nbin_angle, true); }
fd_hash_consts fd_make_consts(const fd_hash_params *p) { return make_consts(p); }
// configuration k of the --multiple-bins list (k < n_multiple_bins), or the single configuration when the list is empty
uint32_t fd_num_bin_configs(const fd_hash_params *p) { return p->n_multiple_bins ? p->n_multiple_bins : 1u; }
fd_hash_consts fd_make_consts_cfg(const fd_hash_params *p, uint32_t k) {
    if (!p->n_multiple_bins) return make_consts(p);
    return make_consts_bins(p, p->multiple_bins[k][0], p->multiple_bins[k][1], false);
}
bool fd_multiple_bins_valid(const fd_hash_params *p) {
    if (p->n_multiple_bins > FDGPU_MAX_MULTIPLE_BINS) return false;
    for (uint32_t k = 0; k < p->n_multiple_bins; ++k)
        if (p->multiple_bins[k][0] == 0 || p->multiple_bins[k][1] == 0) return false;
    return true;
}

int d2h_u64(fdgpu_ctx *c, const uint64_t *dev, uint64_t *host) {
    HIPCHK(c, hipMemcpyAsync(host, dev, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FDGPU_OK;
}

// stable sort of (keys, vals) by the low key_bits of keys
int sort_pairs(fdgpu_ctx *c, uint32_t *ka, uint32_t *va, uint32_t *kb, uint32_t *vb, uint64_t n, int key_bits) {
    return fd_radix_sort_pairs(ka, va, kb, vb, n, key_bits, c->ws[WS_GHIST].as<uint32_t>(), c->ws[WS_TOT].as<uint64_t>(), c->stream, c);
}

// ---- S2: the index object (the build that fills it: fd_api_build.hip) --------------------------------------------------
// An index's blocks come from the pool of the context that owns it (steady-state builds then call neither hipMalloc nor hipFree, which would
// serialise the stream), or from hipMalloc for an index without one (fdgpu_index_load); fdgpu_index_destroy releases them the same way.
hipError_t fd_index_block(fdgpu_ctx *pool, size_t bytes, void **p, size_t *cap) {
    if (!pool) return hipMalloc(p, bytes);
    hipError_t e;
    *p = pool->pool_alloc(bytes, &e);
    *cap = pool->last_cap;
    return e;
}
int fd_index_new(fdgpu_ctx *c, bool pooled, uint64_t H, uint64_t value_len, bool with_last, fdgpu_index **out) {
    *out = nullptr;
    fdgpu_index *ix = new (std::nothrow) fdgpu_index();
    if (!ix) FAIL(c, FDGPU_ENOMEM, "index alloc: out of memory");
    ix->ctx = pooled ? c : nullptr; ix->n_hashes = H;
    hipError_t e = hipSuccess;
    if (value_len != FD_VALUE_LATER) { ix->value_len = value_len; e = fd_index_block(ix->ctx, value_len + FD_VALUE_SLACK, (void **)&ix->value, &ix->cap_value); }
    if (e == hipSuccess) e = fd_index_block(ix->ctx, std::max<uint64_t>(H, 1) * 4, (void **)&ix->hashes, &ix->cap_hashes);
    if (e == hipSuccess) e = fd_index_block(ix->ctx, (H + 1) * 8, (void **)&ix->offsets, &ix->cap_offsets);
    if (e == hipSuccess && with_last) e = fd_index_block(ix->ctx, std::max<uint64_t>(H, 1) * 4, (void **)&ix->last_ids, &ix->cap_last);
    if (e != hipSuccess) { c->err = std::string("index alloc: ") + hipGetErrorString(e); fdgpu_index_destroy(ix); return FDGPU_EHIP; }
    *out = ix;
    return FDGPU_OK;
}
__global__ void k_ix_order(const uint8_t *__restrict__ sel, const uint8_t *__restrict__ is_long, const uint64_t *__restrict__ sel_pre,
                           const uint64_t *__restrict__ long_pre, uint64_t H, uint32_t *__restrict__ order, uint32_t *__restrict__ place) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= H || (sel && !sel[t])) return;
    const uint64_t n_long = long_pre[H];
    const uint64_t g = is_long[t] ? long_pre[t] : n_long + ((sel ? sel_pre[t] : t) - long_pre[t]);
    order[g] = (uint32_t)t;
    if (place) place[t] = (uint32_t)g;
}
void fd_order_long_first(const uint8_t *sel, const uint8_t *is_long, uint64_t H, uint64_t *sel_pre, uint64_t *long_pre, uint64_t *scan_tmp,
                         uint64_t *total_dev, uint32_t *order, uint32_t *place, hipStream_t st) {
    if (sel) fd_exclusive_scan<uint8_t>(sel, H, sel_pre, scan_tmp, total_dev, st);
    fd_exclusive_scan<uint8_t>(is_long, H, long_pre, scan_tmp, total_dev, st);
    hipLaunchKernelGGL(k_ix_order, dim3(fd_grid(H, 256)), dim3(256), 0, st, sel, is_long, sel_pre, long_pre, H, order, place);
}
extern "C" void fdgpu_index_destroy(fdgpu_index *ix) {
    if (!ix) return;
    FD_LOCK(ix->ctx);     // the blocks go back to the context's pool
    if (ix->ctx) {
        ix->ctx->pool_free(ix->hashes, ix->cap_hashes); ix->ctx->pool_free(ix->offsets, ix->cap_offsets); ix->ctx->pool_free(ix->value, ix->cap_value);
    } else { (void)hipFree(ix->hashes); (void)hipFree(ix->offsets); (void)hipFree(ix->value); }
    if (ix->ctx && ix->cap_last) ix->ctx->pool_free(ix->last_ids, ix->cap_last);
    else (void)hipFree(ix->last_ids);      // no context, or derived later by fd_index_last_ids
    if (ix->penalty) (void)hipFree(ix->penalty);
    if (ix->lens) (void)hipFree(ix->lens);
    if (ix->ck_meta) (void)hipFree(ix->ck_meta);
    if (ix->ck_ent) (void)hipFree(ix->ck_ent);
    delete ix;
}
extern "C" int fdgpu_index_set_first_id(fdgpu_index *ix, uint64_t first_id) { if (!ix || first_id + ix->n_structures > 0xffffffffull) return FDGPU_EINVAL; ix->first_id = first_id; return FDGPU_OK; }
extern "C" uint64_t fdgpu_index_num_hashes(const fdgpu_index *ix) { return ix ? ix->n_hashes : 0; }
extern "C" uint64_t fdgpu_index_value_len(const fdgpu_index *ix) { return ix ? ix->value_len : 0; }
extern "C" uint64_t fdgpu_index_num_postings(const fdgpu_index *ix) { return ix ? ix->n_postings : 0; }
extern "C" uint64_t fdgpu_index_num_structures(const fdgpu_index *ix) { return ix ? ix->n_structures : 0; }

// A large device-to-host copy into ordinary (pageable) memory.  The runtime's own path stages through one internal buffer and one
// host thread (~12 GB/s: 2.2 s for the 26 GB of a Swiss-Prot-scale index); here FD_PIN_SLOTS pinned buffers are filled by
// asynchronous copies on the context's stream and emptied by as many host threads, which also take the destination's first-touch
// page faults in parallel (the destination is asked for huge pages).
#define FD_PIN_SLOTS 16
#define FD_PIN_BYTES ((size_t)16 << 20)
hipError_t fd_d2h_big(fdgpu_ctx *c, void *dst, const void *src, size_t bytes) {
    if (bytes < 4 * FD_PIN_BYTES) return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    for (int k = 0; k < FD_PIN_SLOTS; ++k) {
        hipError_t e = hipSuccess;
        if (!c->pin[k]) e = hipHostMalloc(&c->pin[k], FD_PIN_BYTES, hipHostMallocDefault);
        if (e == hipSuccess && !c->pin_ev[k]) e = hipEventCreateWithFlags(&c->pin_ev[k], hipEventDisableTiming);
        if (e != hipSuccess) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);      // no pinned memory: the plain path
    }
    {   // transparent huge pages for the destination, where the kernel offers them (a hint: ignoring failure is correct)
        const uintptr_t a = ((uintptr_t)dst + 0x1fffff) & ~(uintptr_t)0x1fffff, b = ((uintptr_t)dst + bytes) & ~(uintptr_t)0x1fffff;
        if (b > a) (void)madvise((void *)a, b - a, MADV_HUGEPAGE);
    }
    const size_t n_chunks = (bytes + FD_PIN_BYTES - 1) / FD_PIN_BYTES;
    std::vector<std::thread> drain(FD_PIN_SLOTS);
    hipError_t err = hipSuccess;
    const int dev = c->device;
    for (size_t i = 0; i < n_chunks && err == hipSuccess; ++i) {
        const int k = (int)(i % FD_PIN_SLOTS);
        if (drain[k].joinable()) drain[k].join();                  // the slot's previous chunk has left the pinned buffer
        const size_t off = i * FD_PIN_BYTES, n = std::min(FD_PIN_BYTES, bytes - off);
        err = hipMemcpyAsync(c->pin[k], (const uint8_t *)src + off, n, hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipEventRecord(c->pin_ev[k], c->stream);
        if (err != hipSuccess) break;
        void *pin = c->pin[k];
        hipEvent_t ev = c->pin_ev[k];
        drain[k] = std::thread([=]() { (void)hipSetDevice(dev); (void)hipEventSynchronize(ev); memcpy((uint8_t *)dst + off, pin, n); });
    }
    for (auto &t : drain) if (t.joinable()) t.join();
    return err;
}

extern "C" int fdgpu_index_export(fdgpu_ctx *c, const fdgpu_index *ix, uint8_t **value, uint64_t *value_len, uint32_t **hashes,
                                  uint64_t **offsets, uint64_t *n_hashes) { FD_LOCK(c);
    if (!c || !ix || !value || !value_len || !hashes || !offsets || !n_hashes) return FDGPU_EINVAL;
    uint8_t *v = (uint8_t *)malloc(std::max<uint64_t>(ix->value_len, 1));
    uint32_t *h = (uint32_t *)malloc(std::max<uint64_t>(ix->n_hashes, 1) * 4);
    uint64_t *o = (uint64_t *)malloc((ix->n_hashes + 1) * 8);
    if (!v || !h || !o) { free(v); free(h); free(o); return FDGPU_ENOMEM; }
    hipError_t e = fd_d2h_big(c, v, ix->value, ix->value_len);
    if (e == hipSuccess) e = fd_d2h_big(c, h, ix->hashes, ix->n_hashes * 4);
    if (e == hipSuccess) e = fd_d2h_big(c, o, ix->offsets, (ix->n_hashes + 1) * 8);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { free(v); free(h); free(o); c->err = std::string("index export: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    *value = v; *value_len = ix->value_len; *hashes = h; *offsets = o; *n_hashes = ix->n_hashes;
    return FDGPU_OK;
}

extern "C" int fdgpu_index_load(fdgpu_ctx *c, const uint32_t *hashes, const uint64_t *offsets, uint64_t H, const uint8_t *value,
                                uint64_t vlen, uint64_t n_structures, fdgpu_index **out) { FD_LOCK(c);
    if (!c || !out || (H && (!hashes || !offsets)) || (vlen && !value)) return FDGPU_EINVAL;
    *out = nullptr;
    fdgpu_index *ix = nullptr;
    int rc = fd_index_new(c, false, H, vlen, false, &ix);
    if (rc) return rc;
    ix->n_structures = n_structures;
    hipError_t e = hipSuccess;
    uint64_t zero = 0;
    if ((vlen && (e = hipMemcpyAsync(ix->value, value, vlen, hipMemcpyHostToDevice, c->stream)) != hipSuccess) ||
        (H && (e = hipMemcpyAsync(ix->hashes, hashes, H * 4, hipMemcpyHostToDevice, c->stream)) != hipSuccess) ||
        (e = hipMemcpyAsync(ix->offsets, H ? offsets : &zero, (H + 1) * 8, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        c->err = std::string("index load: ") + hipGetErrorString(e);
        fdgpu_index_destroy(ix);
        return FDGPU_EHIP;
    }
    if ((e = fd_count_postings(c, ix->value, vlen, &ix->n_postings)) != hipSuccess) {      // an index that would report 0 postings: refuse it
        (void)hipGetLastError();
        c->err = std::string("index load: counting the postings: ") + hipGetErrorString(e);
        fdgpu_index_destroy(ix);
        return FDGPU_EHIP;
    }
    *out = ix;
    return FDGPU_OK;
}

// byte-identical to wrapup_offset_and_save_entries + save_offset_to_file (indextable.rs:239-264, 297-326)
// Device array -> file region, streamed: chunks of FD_PIN_BYTES land in the context's pinned slots (asynchronous copies on the context's stream) and
// as many host threads pwrite() them straight from the pinned buffer into the file at their own offset — no host copy of the array, and the
// page-cache copies of the chunks run in parallel (export-then-fwrite was one thread copying 976 MB twice: 0.33 of the CLI's 0.73 s at 20,500
// structures).  io_err: first errno of a failed write.
hipError_t fd_d2h_to_file(fdgpu_ctx *c, int fd, uint64_t file_off, const void *src, size_t bytes, std::atomic<int> *io_err) {
    if (!bytes) return hipSuccess;
    for (int k = 0; k < FD_PIN_SLOTS; ++k) {
        hipError_t e = hipSuccess;
        if (!c->pin[k]) e = hipHostMalloc(&c->pin[k], FD_PIN_BYTES, hipHostMallocDefault);
        if (e == hipSuccess && !c->pin_ev[k]) e = hipEventCreateWithFlags(&c->pin_ev[k], hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    const size_t n_chunks = (bytes + FD_PIN_BYTES - 1) / FD_PIN_BYTES;
    std::vector<std::thread> drain(FD_PIN_SLOTS);
    hipError_t err = hipSuccess;
    const int dev = c->device;
    for (size_t i = 0; i < n_chunks && err == hipSuccess; ++i) {
        const int k = (int)(i % FD_PIN_SLOTS);
        if (drain[k].joinable()) drain[k].join();                  // the slot's previous chunk is in the file
        const size_t off = i * FD_PIN_BYTES, n = std::min(FD_PIN_BYTES, bytes - off);
        err = hipMemcpyAsync(c->pin[k], (const uint8_t *)src + off, n, hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipEventRecord(c->pin_ev[k], c->stream);
        if (err != hipSuccess) break;
        const uint8_t *pin = (const uint8_t *)c->pin[k];
        hipEvent_t ev = c->pin_ev[k];
        drain[k] = std::thread([=]() {
            (void)hipSetDevice(dev);
            if (hipEventSynchronize(ev) != hipSuccess) { int z = 0; io_err->compare_exchange_strong(z, EIO); return; }
            size_t done = 0;
            while (done < n) {
                const ssize_t w = pwrite(fd, pin + done, n - done, (off_t)(file_off + off + done));
                if (w < 0) { if (errno == EINTR) continue; int z = 0; io_err->compare_exchange_strong(z, errno ? errno : EIO); return; }
                done += (size_t)w;
            }
        });
    }
    for (auto &t : drain) if (t.joinable()) t.join();
    return err;
}

// The page-locked staging slots of fdgpu_index_save / _save_part / _export (16 x 16 MB), made now instead of inside the first of those calls: a host that
// knows it will write an index (the index command) calls this while its first chunk is still being parsed — page-locking 256 MB is ~20 ms.
extern "C" int fdgpu_reserve_staging(fdgpu_ctx *c) { FD_LOCK(c);
    if (!c) return FDGPU_EINVAL;
    for (int k = 0; k < FD_PIN_SLOTS; ++k) {
        if (!c->pin[k]) HIPCHK(c, hipHostMalloc(&c->pin[k], FD_PIN_BYTES, hipHostMallocDefault));
        if (!c->pin_ev[k]) HIPCHK(c, hipEventCreateWithFlags(&c->pin_ev[k], hipEventDisableTiming));
    }
    return FDGPU_OK;
}

// PREFIX (value bytes) and PREFIX.offset (u64 H | u32 hashes[H] | u64 offsets[H + 1]) — byte-identical to save_offset_to_file /
// wrapup_offset_and_save_entries (src/index/indextable.rs:239-326), written straight from the device arrays
extern "C" int fdgpu_index_save(fdgpu_ctx *c, const fdgpu_index *ix, const char *prefix) { FD_LOCK(c);
    if (!c || !ix || !prefix) return FDGPU_EINVAL;
    const std::string p(prefix);
    const uint64_t H = ix->n_hashes;
    std::atomic<int> io_err{0};
    hipError_t e = hipSuccess;
    const int fv = open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    const int fo = fv >= 0 ? open((p + ".offset").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644) : -1;
    if (fv < 0 || fo < 0) { if (fv >= 0) close(fv); FAIL(c, FDGPU_EINVAL, "index save: cannot write " + p); }
    if (pwrite(fo, &H, 8, 0) != 8) io_err = errno ? errno : EIO;
    const bool trace = getenv("FDGPU_TRACE") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    if (trace) {      // measurement aid: the page-locking of the staging slots apart from the streaming
        for (int k = 0; k < FD_PIN_SLOTS && e == hipSuccess; ++k) if (!c->pin[k]) e = hipHostMalloc(&c->pin[k], FD_PIN_BYTES, hipHostMallocDefault);
        fprintf(stderr, "[index_save] staging slots page-locked at %.3f ms\n", ms());
    }
    if (e == hipSuccess) e = fd_d2h_to_file(c, fv, 0, ix->value, ix->value_len, &io_err);
    if (trace) fprintf(stderr, "[index_save] %llu value bytes streamed at %.3f ms\n", (unsigned long long)ix->value_len, ms());
    if (e == hipSuccess) e = fd_d2h_to_file(c, fo, 8, ix->hashes, H * 4, &io_err);
    if (e == hipSuccess) e = fd_d2h_to_file(c, fo, 8 + H * 4, ix->offsets, (H + 1) * 8, &io_err);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (trace) fprintf(stderr, "[index_save] offset file streamed at %.3f ms\n", ms());
    if (close(fv) != 0 && !io_err) io_err = errno ? errno : EIO;
    if (close(fo) != 0 && !io_err) io_err = errno ? errno : EIO;
    if (trace) fprintf(stderr, "[index_save] files closed at %.3f ms\n", ms());
    if (e != hipSuccess) { c->err = std::string("index save: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    if (io_err) FAIL(c, FDGPU_EINVAL, "index save: cannot write " + p + " (" + strerror(io_err) + ")");
    return FDGPU_OK;
}

// ---- diagnostics --------------------------------------------------------------------------------------------------------
__global__ void k_debug_libm(int op, const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ out, uint64_t n) {
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float x = a[k], s, c;
    switch (op) {
        case 0: fdd_sincosf(x, &s, &c); out[k] = s; break;
        case 1: fdd_sincosf(x, &s, &c); out[k] = c; break;
        case 2: out[k] = fdd_acosf(x); break;
        case 3: out[k] = fdd_atanf(x); break;
        default: out[k] = fdd_atan2f(x, b[k]); break;
    }
}
extern "C" int fdgpu_debug_libm(fdgpu_ctx *c, int op, const float *a, const float *b, float *out, uint64_t n) { FD_LOCK(c);
    if (!c || !a || !out || (op == 4 && !b) || op < 0 || op > 4) return FDGPU_EINVAL;
    if (!n) return FDGPU_OK;
    hipStream_t st = c->stream;
    HIPCHK(c, c->ws[WS_MISC0].ensure(n * 4));
    HIPCHK(c, c->ws[WS_MISC1].ensure(n * 4));
    HIPCHK(c, c->ws[WS_MISC2].ensure(n * 4));
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC0].p, a, n * 4, hipMemcpyHostToDevice, st));
    if (b) HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC1].p, b, n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_debug_libm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, op, c->ws[WS_MISC0].as<float>(),
                       c->ws[WS_MISC1].as<float>(), c->ws[WS_MISC2].as<float>(), n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->ws[WS_MISC2].p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDGPU_OK;
}
