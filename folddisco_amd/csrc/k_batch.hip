// k_batch.hip — operations on a resident batch (the coordinates an index is paired with): fdgpu_batch_select, fdgpu_batch_concat,
// fdgpu_batch_export.  They are the batch counterparts of the id-mapping index operations: remove / permute / split of an index
// pair with a select of its batch, a merge with a concat.  Bytes are moved, never re-derived: retrieval hashes these coordinates.
//
//   k_batch_select   one wavefront per OUTPUT work item, i.e. per (structure, 64-residue tile) of the result — the items the output batch needs
//                    anyway (fd_build_work_items).  The tile's residues are one contiguous run in the source as well, so the wavefront copies
//                    three runs of up to 192 dwords (lane t, t + 64, t + 128: consecutive lanes, consecutive dwords) and two runs of up to 64
//                    bytes (lane per byte).  A coordinate run starts at byte 12 * r: dword-aligned only, so the accesses are 4 bytes wide.
//                    Addresses come from res_off and ids alone, both bounded on the host before the launch; no atomics, no LDS, no cross-lane
//                    traffic.  HBM-bound: every byte once in, once out.
//   concat           device-to-device copies at running offsets, no kernel; a part without cb_valid contributes ones when another part has it
//   export           the five arrays back to the host, res_off from the batch's host copy
#include "fdgpu_internal.h"
#include "fd_api_common.h"
#include <string.h>
#include <stdlib.h>

struct bs_args {
    const float *s_n, *s_ca, *s_cb; const uint8_t *s_aa, *s_cbv;      // source batch (s_cbv null: none)
    float *d_n, *d_ca, *d_cb; uint8_t *d_aa, *d_cbv;                 // output batch
    const uint32_t *s_off, *d_off;                                   // res_off of the source [S + 1] and of the output [n + 1]
    const uint32_t *ids;                                             // [n] source structure of every output structure (all < S: checked on the host)
    const uint32_t *wi_struct, *wi_i0;                               // the output's work items: structure, first residue (absolute) of the tile
    uint32_t n_work;
};

__global__ __launch_bounds__(256) void k_batch_select(bs_args A) {
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= A.n_work) return;
    const uint32_t k = A.wi_struct[w], d0 = A.wi_i0[w];
    const uint32_t n = min(A.d_off[k + 1] - d0, (uint32_t)FD_WAVE);      // residues of the tile: 1 .. 64, inside output structure k
    const uint64_t s0 = (uint64_t)A.s_off[A.ids[k]] + (d0 - A.d_off[k]);  // the same residues in the source: structure ids[k] has the same length
    const uint64_t sx = 3 * s0, dx = 3 * (uint64_t)d0;
    for (uint32_t t = lane; t < 3 * n; t += FD_WAVE) {
        A.d_n[dx + t] = A.s_n[sx + t];
        A.d_ca[dx + t] = A.s_ca[sx + t];
        A.d_cb[dx + t] = A.s_cb[sx + t];
    }
    if (lane < n) {
        A.d_aa[d0 + lane] = A.s_aa[s0 + lane];
        if (A.s_cbv) A.d_cbv[d0 + lane] = A.s_cbv[s0 + lane];
    }
}

// an owning batch with room for R residues (with_cbv: and their cb_valid); res_off is the caller's
static int batch_alloc(fdgpu_ctx *c, uint64_t n_struct, uint64_t R, bool with_cbv, fdgpu_batch **out) {
    fdgpu_batch *b = new (std::nothrow) fdgpu_batch();
    if (!b) return FDGPU_ENOMEM;
    *out = b;
    b->ctx = c; b->owns = true; b->n_struct = n_struct; b->n_res = R;
    HIPCHK(c, hipMalloc((void **)&b->n_xyz, std::max<size_t>(R * 12, 4)));
    HIPCHK(c, hipMalloc((void **)&b->ca_xyz, std::max<size_t>(R * 12, 4)));
    HIPCHK(c, hipMalloc((void **)&b->cb_xyz, std::max<size_t>(R * 12, 4)));
    HIPCHK(c, hipMalloc((void **)&b->aa, std::max<size_t>(R, 4)));
    if (with_cbv) HIPCHK(c, hipMalloc((void **)&b->cb_valid, std::max<size_t>(R, 4)));
    return FDGPU_OK;
}

static int select_impl(fdgpu_ctx *c, const fdgpu_batch *b, const uint32_t *ids, uint64_t n, fdgpu_batch **out) {
    hipStream_t st = c->stream;
    // everything the kernel will use as an address is settled here: ids against n_struct, the output's res_off from the source's host copy
    uint64_t tot = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (ids[k] >= b->n_struct) {
            char m[160];
            snprintf(m, sizeof m, "batch select: ids[%llu] = %u, the batch holds %llu structures", (unsigned long long)k, ids[k], (unsigned long long)b->n_struct);
            FAIL(c, FDGPU_EINVAL, m);
        }
        tot += b->h_res_off[ids[k] + 1] - b->h_res_off[ids[k]];      // 64-bit: repeats can pass 2^32 (a structure has at most 65,535 residues, n is below 2^32)
    }
    if (tot >= 0xffffffffull) FAIL(c, FDGPU_ERANGE, "batch select: more than 2^32 residues in the selected batch");
    std::vector<uint64_t> off(n + 1);
    off[0] = 0;
    for (uint64_t k = 0; k < n; ++k) off[k + 1] = off[k] + (b->h_res_off[ids[k] + 1] - b->h_res_off[ids[k]]);
    const uint64_t R = off[n];
    fdgpu_batch *nb = nullptr;
    int rc = batch_alloc(c, n, R, b->cb_valid != nullptr, &nb);
    *out = nb;
    if (rc) return rc;
    nb->h_res_off.swap(off);
    if ((rc = fd_build_work_items(c, nb, /*with_hash_ok=*/false))) return rc;      // res_off and the work items on the device; hash_ok allocated
    if (nb->n_work) {
        HIPCHK(c, c->ws[WS_MISC0].ensure(n * 4));
        uint32_t *d_ids = c->ws[WS_MISC0].as<uint32_t>();
        HIPCHK(c, hipMemcpyAsync(d_ids, ids, n * 4, hipMemcpyHostToDevice, st));
        bs_args A{b->n_xyz, b->ca_xyz, b->cb_xyz, b->aa, b->cb_valid, nb->n_xyz, nb->ca_xyz, nb->cb_xyz, nb->aa, nb->cb_valid,
                  b->res_off, nb->res_off, d_ids, nb->wi_struct, nb->wi_i0, nb->n_work};
        StageTimer t(c, "batch_select", 2 * R * (36 + 1 + (b->cb_valid ? 1 : 0)) + (uint64_t)nb->n_work * 20);
        hipLaunchKernelGGL(k_batch_select, dim3(fd_grid(nb->n_work, 4)), dim3(256), 0, st, A);
    }
    HIPCHK(c, hipGetLastError());
    fd_launch_hash_ok(nb->aa, nb->cb_valid, nb->hash_ok, nb->n_res, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));      // ids is the caller's, and the workspace is free again, when the call returns
    return FDGPU_OK;
}

extern "C" int fdgpu_batch_select(fdgpu_ctx *c, const fdgpu_batch *b, const uint32_t *ids, uint64_t n, fdgpu_batch **out) { FD_LOCK(c);
    if (!c || !b || !out || (n && !ids)) return FDGPU_EINVAL;
    *out = nullptr;
    if (n >= 0xffffffffull) FAIL(c, FDGPU_ERANGE, "batch select: too many structures in one batch");
    reset_timings(c);
    fdgpu_batch *nb = nullptr;
    const int rc = select_impl(c, b, ids, n, &nb);
    if (rc != FDGPU_OK) {
        (void)hipStreamSynchronize(c->stream);
        fdgpu_batch_destroy(nb);
        return rc;
    }
    *out = nb;
    return FDGPU_OK;
}

// the parts' arrays into nb at running residue offsets (and nb's host res_off); timed as one stage, without the work items that follow
static int concat_copies(fdgpu_ctx *c, const fdgpu_batch *const *parts, uint64_t n_parts, fdgpu_batch *nb, bool any_cbv) {
    hipStream_t st = c->stream;
    StageTimer t(c, "batch_concat", 2 * nb->n_res * (36 + 1 + (any_cbv ? 1 : 0)));
    uint64_t r0 = 0;
    for (uint64_t p = 0; p < n_parts; ++p) {
        const fdgpu_batch *q = parts[p];
        for (uint64_t s = 1; s <= q->n_struct; ++s) nb->h_res_off.push_back(r0 + q->h_res_off[s]);
        if (q->n_res) {
            HIPCHK(c, hipMemcpyAsync(nb->n_xyz + 3 * r0, q->n_xyz, q->n_res * 12, hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpyAsync(nb->ca_xyz + 3 * r0, q->ca_xyz, q->n_res * 12, hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpyAsync(nb->cb_xyz + 3 * r0, q->cb_xyz, q->n_res * 12, hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpyAsync(nb->aa + r0, q->aa, q->n_res, hipMemcpyDeviceToDevice, st));
            if (q->cb_valid) HIPCHK(c, hipMemcpyAsync(nb->cb_valid + r0, q->cb_valid, q->n_res, hipMemcpyDeviceToDevice, st));
            else if (any_cbv) HIPCHK(c, hipMemsetAsync(nb->cb_valid + r0, 1, q->n_res, st));      // NULL = all 1 (fd_batch_desc)
        }
        r0 += q->n_res;
    }
    return FDGPU_OK;
}

static int concat_impl(fdgpu_ctx *c, const fdgpu_batch *const *parts, uint64_t n_parts, fdgpu_batch **out) {
    uint64_t S = 0, R = 0;
    bool any_cbv = false;
    for (uint64_t p = 0; p < n_parts; ++p) { S += parts[p]->n_struct; R += parts[p]->n_res; any_cbv = any_cbv || parts[p]->cb_valid != nullptr; }
    if (S >= 0xffffffffull) FAIL(c, FDGPU_ERANGE, "batch concat: too many structures in one batch");
    if (R >= 0xffffffffull) FAIL(c, FDGPU_ERANGE, "batch concat: more than 2^32 residues in one batch");
    fdgpu_batch *nb = nullptr;
    int rc = batch_alloc(c, S, R, any_cbv, &nb);
    *out = nb;
    if (rc) return rc;
    nb->h_res_off.reserve(S + 1);
    nb->h_res_off.push_back(0);
    if ((rc = concat_copies(c, parts, n_parts, nb, any_cbv))) return rc;
    return fd_build_work_items(c, nb);      // stream-ordered behind the copies; synchronises
}

extern "C" int fdgpu_batch_concat(fdgpu_ctx *c, const fdgpu_batch *const *parts, uint64_t n_parts, fdgpu_batch **out) { FD_LOCK(c);
    if (!c || !parts || !out) return FDGPU_EINVAL;
    *out = nullptr;
    if (n_parts < 2 || n_parts > 64) FAIL(c, FDGPU_EINVAL, "batch concat: 2 to 64 parts are joined in one call");
    for (uint64_t p = 0; p < n_parts; ++p)
        if (!parts[p]) FAIL(c, FDGPU_EINVAL, "batch concat: a part is NULL");
    reset_timings(c);
    fdgpu_batch *nb = nullptr;
    const int rc = concat_impl(c, parts, n_parts, &nb);
    if (rc != FDGPU_OK) {
        (void)hipStreamSynchronize(c->stream);
        fdgpu_batch_destroy(nb);
        return rc;
    }
    *out = nb;
    return FDGPU_OK;
}

extern "C" int fdgpu_batch_export(fdgpu_ctx *c, const fdgpu_batch *b, fd_batch_desc *h) { FD_LOCK(c);
    if (!c || !b || !h) return FDGPU_EINVAL;
    memset(h, 0, sizeof *h);
    const uint64_t R = b->n_res, S = b->n_struct;
    uint64_t *off = (uint64_t *)malloc((S + 1) * 8);
    float *nx = (float *)malloc(std::max<size_t>(R * 12, 4)), *ca = (float *)malloc(std::max<size_t>(R * 12, 4)), *cb = (float *)malloc(std::max<size_t>(R * 12, 4));
    uint8_t *aa = (uint8_t *)malloc(std::max<size_t>(R, 1)), *cbv = b->cb_valid ? (uint8_t *)malloc(std::max<size_t>(R, 1)) : nullptr;
    auto drop = [&] { free(off); free(nx); free(ca); free(cb); free(aa); free(cbv); };
    if (!off || !nx || !ca || !cb || !aa || (b->cb_valid && !cbv)) { drop(); return FDGPU_ENOMEM; }
    memcpy(off, b->h_res_off.data(), (S + 1) * 8);
    hipError_t e = hipSuccess;
    if (R) {
        e = hipMemcpyAsync(nx, b->n_xyz, R * 12, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ca, b->ca_xyz, R * 12, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(cb, b->cb_xyz, R * 12, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(aa, b->aa, R, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && cbv) e = hipMemcpyAsync(cbv, b->cb_valid, R, hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { drop(); c->err = std::string("batch export: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    h->n_struct = S; h->res_off = off; h->n_xyz = nx; h->ca_xyz = ca; h->cb_xyz = cb; h->aa = aa; h->cb_valid = cbv;
    return FDGPU_OK;
}
