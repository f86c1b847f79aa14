// fd_query_map.hip — make_query_map behind the C ABI (src/controller/query.rs:208-329, helpers :53-206): pair features and hashes on the GPU
// (k_pair_features*, k_hash_features, the device chain k_qm_expand_hash / k_qm_dedupe / posting-length lookup for motif batches and whole-structure
// queries), expansion / substitution / first-insert-wins bookkeeping and the assembly of the fd_query_map blocks on the host.
// The reference is compiled code, so this glue is C++ behind the same C ABI; it contains no f32 arithmetic that decides a hash bit (that all
// happens in the kernels) except the query expansion's feature +- delta adds, which are single IEEE f32 adds exactly like the reference's.
// (Split from fd_host_query.hip, which keeps the retrieval glue.)
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>
#include "fdgpu_internal.h"
#include "fd_query_map_host.h"

#define HIPCHK(ctx, expr)                                                                                   \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) {                                                                             \
            char _b[512];                                                                                   \
            snprintf(_b, sizeof _b, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));  \
            (ctx)->err = _b;                                                                                \
            return FDGPU_EHIP;                                                                              \
        }                                                                                                   \
    } while (0)

fd_hash_consts fd_make_consts(const fd_hash_params *p);  // fdgpu_api.hip
fd_hash_consts fd_make_consts_cfg(const fd_hash_params *p, uint32_t k);
uint32_t fd_num_bin_configs(const fd_hash_params *p);
bool fd_multiple_bins_valid(const fd_hash_params *p);
bool fd_hash_type_supported(uint32_t t);
#define CHECK_TYPE(ctx, p)                                                                                                       \
    do {                                                                                                                         \
        if (!fd_hash_type_supported((p)->hash_type)) {                                                                           \
            (ctx)->err = "hash_type: only the encodings over the (d_CA, d_CB, theta, tau1, tau2) descriptor are built (0, 1, 3, 7, 8)"; \
            return FDGPU_EINVAL;                                                                                                 \
        }                                                                                                                        \
    } while (0)

// ------------------------------------------------------------------------------------------ kernels
// get_single_feature (src/controller/feature.rs:11-24, 84-99) for explicit residue pairs of one structure
__global__ void k_pair_features(fd_batch_view B, uint32_t s, const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pj, uint32_t n,
                                float cutoff, uint32_t type, float *__restrict__ feat /*[n][7]*/, uint8_t *__restrict__ valid) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    // s == 0xffffffff: pi / pj are residue indices of the whole batch (pairs of many structures in one launch)
    const uint32_t r0 = s == 0xffffffffu ? 0u : B.res_off[s], r1 = s == 0xffffffffu ? B.res_off[B.n_struct] : B.res_off[s + 1];
    uint32_t i = r0 + pi[k], j = r0 + pj[k];
    bool ok = i < r1 && j < r1 && i != j && B.hash_ok[i] && B.hash_ok[j];
    fd_feature f = {0, 0, 0, 0, 0};
    if (ok) {
        fd_v3 ca1 = fd_load3(B.ca_xyz, i), ca2 = fd_load3(B.ca_xyz, j);
        float d = fd_dist(ca1, ca2);
        if (d > cutoff) ok = false;
        else f = fd_pair_feature(fd_load3(B.n_xyz, i), ca1, fd_load3(B.cb_xyz, i), fd_load3(B.n_xyz, j), ca2, fd_load3(B.cb_xyz, j));
    }
    valid[k] = ok ? 1 : 0;
    float *o = feat + 7ull * k;
    o[0] = ok ? (float)B.aa[i] : 0.f; o[1] = ok ? (float)B.aa[j] : 0.f;
    o[2] = f.ca_dist; o[3] = f.cb_dist; o[4] = type == FD_HASH_PDBMOTIF ? fd_to_degrees(f.angle) : f.angle; o[5] = f.tor1; o[6] = f.tor2;
}
// the same for every encoding, in the query map's own record: [0..9) the feature container of get_single_feature, [9] the CA
// distance and [10], [11] the two residue types (get_list_amino_acids_and_distances, structure/core.rs:462-477 — what the
// observed-distance map holds whatever the encoding puts into the container); FD_QF floats (fd_query_map_host.h)
__global__ void k_pair_features12(fd_batch_view B, const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pj, uint32_t n, float cutoff,
                                  uint32_t type, float *__restrict__ feat /*[n][FD_QF]*/, uint8_t *__restrict__ valid) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t R = B.res_off[B.n_struct];
    const uint32_t i = pi[k], j = pj[k];      // residue indices of the whole batch
    float *o = feat + (uint64_t)FD_QF * k;
    for (int z = 0; z < FD_QF; ++z) o[z] = 0.f;
    bool ok = i < R && j < R && i != j && B.aa[i] != 255 && B.aa[j] != 255;
    if (ok) {
        o[9] = fd_dist(fd_load3(B.ca_xyz, i), fd_load3(B.ca_xyz, j)); o[10] = (float)B.aa[i]; o[11] = (float)B.aa[j];
        if (fd_own_descriptor(type)) {
            uint32_t lo = 0, hi = B.n_struct;                  // structure of residue i: res_off[lo] <= i < res_off[lo + 1]
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (B.res_off[mid] <= i) lo = mid; else hi = mid; }
            const uint32_t r0 = B.res_off[lo], r1 = B.res_off[lo + 1];
            float f[FD_NFEAT];
            ok = j >= r0 && j < r1 && fd_feature_other(type, B, r0, r1, i, j, cutoff, f);
            if (ok) for (int z = 0; z < FD_NFEAT; ++z) o[z] = f[z];
        } else {
            ok = B.hash_ok[i] && B.hash_ok[j] && !(o[9] > cutoff);
            if (ok) {
                const fd_feature f = fd_pair_feature(fd_load3(B.n_xyz, i), fd_load3(B.ca_xyz, i), fd_load3(B.cb_xyz, i), fd_load3(B.n_xyz, j),
                                                     fd_load3(B.ca_xyz, j), fd_load3(B.cb_xyz, j));
                o[0] = o[10]; o[1] = o[11]; o[2] = f.ca_dist; o[3] = f.cb_dist; o[4] = type == FD_HASH_PDBMOTIF ? fd_to_degrees(f.angle) : f.angle;
                o[5] = f.tor1; o[6] = f.tor2;
            }
        }
    }
    valid[k] = ok ? 1 : 0;
}
// GeometricHash::perfect_hash (src/geometry/core.rs:213-246 -> pdb_tr.rs:21-75 and the other encodings) on explicit feature vectors
__global__ void k_hash_features(const float *__restrict__ feat, uint64_t n, uint32_t stride, fd_quant q, uint32_t *__restrict__ out) {
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float *f = feat + (uint64_t)stride * k;
    if (fd_own_descriptor(q.type)) { out[k] = fd_hash_other(q.type, f, q); return; }
    fd_feature ft = {f[2], f[3], f[4], f[5], f[6]};
    out[k] = fd_hash_enc_feat(fd_sat_u32(f[0]), fd_sat_u32(f[1]), ft, q);
}

// Large queries without substitutions (whole-structure queries: ~10^5 pairs, 3.7 candidates each): expand_and_insert (query.rs:179-206) per valid
// pair on the device — the observed container, then near / far per threshold and field in the reference's order, with its f32 restore drift —
// and the hash of every candidate; nothing but the hashes leaves the kernel.  out[v * per_pair + c], c in insertion order.
struct qm_expand_par {
    int di[2], ndi, ai[7], nai;
    float dthr[8], athr[8];
    uint32_t n_dist, n_angle, per_pair;
};
__device__ __forceinline__ uint32_t qm_hash_of(const float *f, const fd_quant &q) {
    if (fd_own_descriptor(q.type)) return fd_hash_other(q.type, f, q);
    fd_feature ft = {f[2], f[3], f[4], f[5], f[6]};
    return fd_hash_enc_feat(fd_sat_u32(f[0]), fd_sat_u32(f[1]), ft, q);
}
__global__ void k_qm_expand_hash(const float *__restrict__ feat, const uint32_t *__restrict__ vp, uint32_t n_valid, qm_expand_par P, fd_quant q,
                                 uint32_t *__restrict__ out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_valid) return;
    const float *f = feat + (uint64_t)FD_QF * vp[v];
    float near[FD_QF], far[FD_QF];
    for (int z = 0; z < FD_QF; ++z) { near[z] = f[z]; far[z] = f[z]; }
    uint32_t *o = out + (uint64_t)v * P.per_pair;
    *o++ = qm_hash_of(near, q);
    for (int grp = 0; grp < 2; ++grp) {
        const int *idxs = grp ? P.ai : P.di;
        const int n_idx = grp ? P.nai : P.ndi;
        const float *thr = grp ? P.athr : P.dthr;
        const uint32_t n_thr = grp ? P.n_angle : P.n_dist;
        for (uint32_t z2 = 0; z2 < n_thr; ++z2)
            for (int z = 0; z < n_idx; ++z) {
                const int idx = idxs[z];
                // the container field by a run-time index: a select chain over the twelve registers instead of private memory
                float nv = 0.f, fv = 0.f;
#pragma unroll
                for (int w = 0; w < FD_QF; ++w) { nv = w == idx ? near[w] : nv; fv = w == idx ? far[w] : fv; }
                const float n1 = nv - thr[z2], f1 = fv + thr[z2];
#pragma unroll
                for (int w = 0; w < FD_QF; ++w) { near[w] = w == idx ? n1 : near[w]; far[w] = w == idx ? f1 : far[w]; }
                *o++ = qm_hash_of(near, q);
                *o++ = qm_hash_of(far, q);
                const float n2 = n1 + thr[z2], f2 = f1 - thr[z2];      // the reference restores with += / -= (f32, not an exact inverse): keep the drift
#pragma unroll
                for (int w = 0; w < FD_QF; ++w) { near[w] = w == idx ? n2 : near[w]; far[w] = w == idx ? f2 : far[w]; }
            }
    }
}
// first insertion wins: after a stable sort of (hash, insertion position) by hash the first element of every run is the hash's earliest insertion
__global__ void k_qm_first(const uint32_t *__restrict__ key, const uint32_t *__restrict__ val, uint64_t n, uint8_t *__restrict__ first) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && (k == 0 || key[k] != key[k - 1])) first[val[k]] = 1;
}
__global__ void k_qm_iota(uint32_t *__restrict__ v, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) v[k] = (uint32_t)k;
}
// first insertion wins, per query of a motif batch: one workgroup per query, its candidates' hashes through an open-addressing table in LDS
// that keeps the SMALLEST insertion position of every hash (a hash always walks the same probe path and slots never empty, so all
// copies of a hash meet in one slot); a candidate is kept when it holds its hash's slot.  Queries of up to QM_DD_MAX candidates.
#define QM_DD_MAX 2048u
#define QM_DD_SLOTS 4096u
__global__ __launch_bounds__(256) void k_qm_dedupe(const uint32_t *__restrict__ hash, const uint64_t *__restrict__ cand_off, uint8_t *__restrict__ first) {
    __shared__ unsigned long long tab[QM_DD_SLOTS];
    const uint64_t c0 = cand_off[blockIdx.x], n = cand_off[blockIdx.x + 1] - c0;
    for (uint32_t k = threadIdx.x; k < QM_DD_SLOTS; k += 256) tab[k] = ~0ull;
    __syncthreads();
    for (uint32_t pos = threadIdx.x; pos < n; pos += 256) {
        const uint32_t h = hash[c0 + pos];
        const unsigned long long mine = ((unsigned long long)h << 32) | pos;
        uint32_t at = (h * 2654435761u) >> 20;      // 12 bits
        for (;;) {
            const unsigned long long old = atomicCAS(&tab[at], ~0ull, mine);
            if (old == ~0ull) break;
            if ((uint32_t)(old >> 32) == h) { atomicMin(&tab[at], mine); break; }
            at = (at + 1u) & (QM_DD_SLOTS - 1u);
        }
    }
    __syncthreads();
    for (uint32_t pos = threadIdx.x; pos < n; pos += 256) {
        const uint32_t h = hash[c0 + pos];
        uint32_t at = (h * 2654435761u) >> 20;
        while ((uint32_t)(tab[at] >> 32) != h) at = (at + 1u) & (QM_DD_SLOTS - 1u);
        first[c0 + pos] = (uint32_t)tab[at] == pos ? 1 : 0;
    }
}
__global__ void k_qm_keep(const uint8_t *__restrict__ first, const uint64_t *__restrict__ pos, uint64_t n, uint32_t *__restrict__ keep) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && first[k]) keep[pos[k]] = (uint32_t)k;
}

extern "C" int fdgpu_pair_features(fdgpu_ctx *c, const fdgpu_batch *b, uint64_t s, const uint32_t *pi, const uint32_t *pj, uint64_t n,
                                   const fd_hash_params *p, float *features, uint8_t *valid) { FD_LOCK(c);
    if (!c || !b || !p || (s >= b->n_struct && s != 0xffffffffull) || (n && (!pi || !pj || !features || !valid))) return FDGPU_EINVAL;
    CHECK_TYPE(c, p);
    if (fd_own_descriptor(p->hash_type)) { c->err = "pair_features: seven-float records hold the PDBTrRosetta descriptor only"; return FDGPU_EINVAL; }
    if (!n) return FDGPU_OK;
    hipStream_t st = c->stream;
    HIPCHK(c, c->ws[WS_MISC0].ensure(n * 4));
    HIPCHK(c, c->ws[WS_MISC1].ensure(n * 4));
    HIPCHK(c, c->ws[WS_MISC2].ensure(n * 28));
    HIPCHK(c, c->ws[WS_MISC3].ensure(n));
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC0].p, pi, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC1].p, pj, n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pair_features, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, b->view(), (uint32_t)s, c->ws[WS_MISC0].as<uint32_t>(),
                       c->ws[WS_MISC1].as<uint32_t>(), (uint32_t)n, p->dist_cutoff, p->hash_type, c->ws[WS_MISC2].as<float>(), c->ws[WS_MISC3].as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(features, c->ws[WS_MISC2].p, n * 28, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(valid, c->ws[WS_MISC3].p, n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDGPU_OK;
}

static int hash_features_q(fdgpu_ctx *c, const float *features, uint64_t n, fd_quant q, uint32_t *hashes, uint32_t stride = 7);
// the single configuration (nbin_dist, nbin_angle; either count 0 -> the encoding's defaults); multiple_bins is not consulted
extern "C" int fdgpu_hash_features(fdgpu_ctx *c, const float *features, uint64_t n, const fd_hash_params *p, uint32_t *hashes) { FD_LOCK(c);
    if (!c || !p || (n && (!features || !hashes))) return FDGPU_EINVAL;
    CHECK_TYPE(c, p);
    if (fd_own_descriptor(p->hash_type)) { c->err = "hash_features: seven-float records hold the PDBTrRosetta descriptor only"; return FDGPU_EINVAL; }
    return hash_features_q(c, features, n, fd_make_consts(p).q, hashes);
}
// internal form of fdgpu_pair_features: batch-wide residue indices, FD_QF floats per pair, every encoding
// land_out != null: the features and flags stay in the context's page-locked block (*land_out = [n x FD_QF floats | n flags]) when it can be had
// — features / valid are then untouched; else they are copied into features / valid
static int pair_features12(fdgpu_ctx *c, const fdgpu_batch *b, const uint32_t *pi, const uint32_t *pj, uint64_t n, const fd_hash_params *p,
                           float *features, uint8_t *valid, uint8_t **land_out = nullptr) {
    if (land_out) *land_out = nullptr;
    if (!n) return FDGPU_OK;
    hipStream_t st = c->stream;
    // one block up ([pi | pj], packed in page-locked memory when it can be had) and one block down ([features | flags]): two copy launches per call, not four
    HIPCHK(c, c->ws[WS_MISC0].ensure(2 * n * 4));
    HIPCHK(c, c->ws[WS_MISC2].ensure(n * 4 * FD_QF + n));
    uint32_t *d_pi = c->ws[WS_MISC0].as<uint32_t>(), *d_pj = d_pi + n;
    uint8_t *d_valid = c->ws[WS_MISC2].as<uint8_t>() + n * 4 * FD_QF;
    uint32_t *up = (uint32_t *)c->host_pinned(FD_HP_PAIRS, 2 * n * 4);
    if (up) {
        memcpy(up, pi, n * 4); memcpy(up + n, pj, n * 4);
        HIPCHK(c, hipMemcpyAsync(d_pi, up, 2 * n * 4, hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(c, hipMemcpyAsync(d_pi, pi, n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(d_pj, pj, n * 4, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_pair_features12, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, b->view(), d_pi, d_pj, (uint32_t)n, p->dist_cutoff, p->hash_type,
                       c->ws[WS_MISC2].as<float>(), d_valid);
    HIPCHK(c, hipGetLastError());
    // page-locked landing block (FD_HP_FEAT, read in place by the caller until its next call): the copy does not stage, one wait, no second copy
    uint8_t *land = land_out ? (uint8_t *)c->host_pinned(FD_HP_FEAT, n * 4 * FD_QF + n) : nullptr;
    if (land) {
        HIPCHK(c, hipMemcpyAsync(land, c->ws[WS_MISC2].p, n * 4 * FD_QF + n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        *land_out = land;
        return FDGPU_OK;
    }
    if (land_out) return FDGPU_OK;      // no page-locked block: the caller asks again with its own arrays
    HIPCHK(c, hipMemcpyAsync(features, c->ws[WS_MISC2].p, n * 4 * FD_QF, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(valid, d_valid, n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDGPU_OK;
}
static int hash_features_q(fdgpu_ctx *c, const float *features, uint64_t n, fd_quant q, uint32_t *hashes, uint32_t stride) {
    if (!n) return FDGPU_OK;
    hipStream_t st = c->stream;
    fd_hash_consts C;
    C.q = q;
    HIPCHK(c, c->ws[WS_MISC2].ensure(n * 4 * stride));
    HIPCHK(c, c->ws[WS_MISC0].ensure(n * 4));
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC2].p, features, n * 4 * stride, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_hash_features, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, c->ws[WS_MISC2].as<float>(), n, stride, C.q, c->ws[WS_MISC0].as<uint32_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hashes, c->ws[WS_MISC0].p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return FDGPU_OK;
}

// ------------------------------------------------------------------------------------------ make_query_map
extern "C" void fdgpu_query_map_free(fd_query_map *m) {
    if (!m) return;
    if (m->arena_bytes) { free(m); return; }       // the map and its arrays are one block (qm_fill_map)
    free(m->hash); free(m->qi); free(m->qj); free(m->is_primary); free(m->idf); free(m->indices); free(m->primary_hash);
    free(m->aad_aa1); free(m->aad_aa2); free(m->aad_dist); free(m->aad_qi);
    free(m->post_len); free(m->post_seg); free(m->post_kidx);
    free(m);
}

// The stages of fdgpu_make_query_map_batch pass these.  The host steps between the kernels are fd_query_map_host.cpp's.
struct qm_request {      // the call's arguments, checked and completed by qm_read_request
    fdgpu_ctx *c; const fdgpu_batch *qb; uint64_t n_queries; const uint32_t *q_struct; const uint64_t *q_off; const uint32_t *q_index;
    const uint8_t *const *subs; const uint32_t *n_subs; const float *dist_thr; uint64_t n_dist; const float *angle_thr_deg; uint64_t n_angle;
    const fd_hash_params *p; const fdgpu_index *index; float total_structures; fd_query_map **out;
    std::vector<float> athr = {};      // the angle thresholds in radians
    bool any_subs = false;             // some residue of the batch has a substitution list
    uint32_t n_cfg = 0;                // --multiple-bins: bin configurations every candidate is inserted under (0: the single one)
    char qd_mode = 0;                  // the forced form, '0' / '1' / '2' (qm_read_request), 0: none
    bool trace = false;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    qm_thresholds thresholds() const { return {dist_thr, n_dist, athr.data(), n_angle}; }
    uint64_t r0(uint64_t t) const { return qb->h_res_off[q_struct[t]]; }      // first residue of query t's structure
};
// Which of the three forms "candidates -> hashes" a call takes:
//   host expansion    substitutions, --multiple-bins, more than 8 thresholds of a kind, 2^31 candidates, no valid pair, forced form '0'
//   device expansion  every candidate's place follows from its pair: the host neither builds nor uploads 48 bytes per candidate.  Then
//     sort-dedupe     ONE query of 32,768 candidates and more (a whole-structure query: ~10^5 pairs, 3 x 10^5 candidates; forced form '1': any size)
//     chain           a motif batch whose queries fit k_qm_dedupe's table (forced form '2': never), with the posting lengths when there is an index
//     hashes only     the rest: first insertions and lengths on the host
struct qm_form {
    bool dev_expand = false, dev_dedupe = false, chain = false, chain_len = false;
    uint64_t per_pair = 0;                   // candidates of a pair without substitutions: observed + near / far per threshold and field
    std::vector<uint64_t> valid_off;         // valid pairs in front of every query
    uint32_t path() const {
        return (dev_expand ? FDGPU_QMPATH_DEVICE_EXPAND : FDGPU_QMPATH_HOST_EXPAND) | (chain ? FDGPU_QMPATH_CHAIN : 0u) | (chain_len ? FDGPU_QMPATH_CHAIN_LENGTHS : 0u) |
               (dev_dedupe ? FDGPU_QMPATH_SORT_DEDUPE : 0u);
    }
};
struct qm_feat_store { std::vector<float> feat; std::vector<uint8_t> valid; };      // the pair features when the landing block cannot be had
struct qm_work {         // the batch's candidates, in the reference's insertion order; query t: [cand_off[t], cand_off[t + 1])
    std::vector<qm_aad> aads;
    std::vector<uint64_t> cand_off;
    uint64_t nc = 0;
    std::vector<uint32_t> vpairs;      // device expansion: the valid pairs, ascending — candidate z is insertion z % per_pair of pair vpairs[z / per_pair]
    qm_cands cands;                    // host expansion: every candidate's container and (residues, observed?, pair)
};
struct qm_hashed {       // candidates -> hashes (+ first-insertion flags, + posting lengths)
    std::vector<uint32_t> hashes;
    std::vector<std::vector<uint32_t>> cfg;      // host form with --multiple-bins: the hashes under every bin pair
    std::vector<const uint32_t *> planes;        // what an insertion's hash is read from: cfg[k], or hashes alone
    std::vector<uint32_t> dev_keep;              // sort-dedupe: the kept positions
    std::vector<uint8_t> land_v;                 // chain: the landing block without page-locked memory
    // the chain's results per candidate (landing block, valid until the call returns); null = not computed
    const uint8_t *ch_first = nullptr; const uint64_t *ch_len = nullptr; const long long *ch_kidx = nullptr; const uint32_t *ch_seg = nullptr;
    qm_insertions insertions(const qm_work &W, uint64_t t) const { return {planes.data(), (uint32_t)planes.size(), W.cand_off[t], (W.cand_off[t + 1] - W.cand_off[t]) * planes.size()}; }
};
struct qm_kept { std::vector<std::vector<uint32_t>> keeps; uint64_t n_keep = 0; };      // per query: insertion positions (candidate * n_cfg + bin pair) that enter the map, ascending
struct qm_lengths {      // per pair: hash and idf of its observed candidate; per kept entry (in query order): posting length, segments, list position
    std::vector<float> pair_idf; std::vector<uint32_t> pair_primary;
    std::vector<uint64_t> ent_len; std::vector<uint32_t> ent_seg; std::vector<long long> ent_kidx;
    const uint64_t *e_len = nullptr; const uint32_t *e_seg = nullptr; const long long *e_kidx = nullptr;      // as the assembly reads them: the vectors, or a landing block
};

// every refusal, ahead of any device work; the only reader of the environment
static int qm_read_request(qm_request &R) {
    fdgpu_ctx *c = R.c;
    if (!c || !R.qb || !R.p || !R.out || !R.q_off || (R.n_queries && !R.q_struct) || (R.q_off[R.n_queries] && !R.q_index)) return FDGPU_EINVAL;
    for (uint64_t t = 0; t < R.n_queries; ++t) { R.out[t] = nullptr; if (R.q_struct[t] >= R.qb->n_struct) return FDGPU_EINVAL; }
    CHECK_TYPE(c, R.p);
    if (!fd_multiple_bins_valid(R.p)) { c->err = "multiple_bins: at most 8 (dist, angle) bin pairs, no zero counts"; return FDGPU_EINVAL; }
    R.n_cfg = R.p->n_multiple_bins;
    const float RADS_PER_DEG = 3.14159274101257324f / 180.0f;  // f32::to_radians
    R.athr.resize(R.n_angle);
    for (uint64_t t = 0; t < R.n_angle; ++t) R.athr[t] = R.angle_thr_deg[t] * RADS_PER_DEG;
    if (R.subs && R.n_subs) for (uint64_t a = 0; a < R.q_off[R.n_queries] && !R.any_subs; ++a) R.any_subs = R.subs[a] != nullptr;
    const char *qd = getenv("FDGPU_QM_DEVICE");      // 0: host form; 1: sort-dedupe for one query of any size; 2: device expansion without the chain (tests compare the forms)
    R.qd_mode = qd ? qd[0] : 0;
    R.trace = getenv("FDGPU_TRACE") != nullptr;
    return FDGPU_OK;
}

// the landing block first; the caller's own arrays only when it cannot be had
static int qm_pair_features(const qm_request &R, const qm_pairs &P, qm_feat_store &S, qm_feat &F) {
    const uint64_t np = P.pi.size();
    uint8_t *land = nullptr;
    int rc = pair_features12(R.c, R.qb, P.pi.data(), P.pj.data(), np, R.p, nullptr, nullptr, &land);
    if (!rc && np && !land) {
        S.feat.resize(np * FD_QF); S.valid.resize(np);
        rc = pair_features12(R.c, R.qb, P.pi.data(), P.pj.data(), np, R.p, S.feat.data(), S.valid.data());
    }
    F = land ? qm_feat{(const float *)land, land + np * 4 * FD_QF} : qm_feat{S.feat.data(), S.valid.data()};
    return rc;
}

// the one place that decides the form (and what fdgpu_debug_last_query_map_path reports)
static qm_form qm_choose_form(const qm_request &R, const qm_pairs &P, const qm_feat &F) {
    qm_form f;
    f.valid_off.assign(R.n_queries + 1, 0);
    uint64_t max_valid = 0;
    for (uint64_t t = 0; t < R.n_queries; ++t) {
        uint64_t nv = 0;
        for (uint64_t k = P.off[t]; k < P.off[t + 1]; ++k) nv += F.valid[k] ? 1 : 0;
        f.valid_off[t + 1] = f.valid_off[t] + nv;
        max_valid = std::max(max_valid, nv);
    }
    const qm_fields fl = qm_fields_of(R.p->hash_type);
    f.per_pair = 1 + 2 * ((uint64_t)fl.ndi * R.n_dist + (uint64_t)fl.nai * R.n_angle);
    const uint64_t n_valid = f.valid_off[R.n_queries], nc = n_valid * f.per_pair;
    const uint64_t qd_min = R.qd_mode == '1' ? 1 : 32768;
    f.dev_expand = !R.any_subs && R.p->n_multiple_bins == 0 && R.n_dist <= 8 && R.n_angle <= 8 && R.qd_mode != '0' && n_valid && nc < (1ull << 31);
    f.dev_dedupe = f.dev_expand && R.n_queries == 1 && nc >= qd_min;
    f.chain = f.dev_expand && !f.dev_dedupe && max_valid * f.per_pair <= QM_DD_MAX && R.qd_mode != '2';
    f.chain_len = f.chain && R.index && R.index->lens && R.index->n_hashes && R.index->n_structures;
    R.c->last_query_map_path = f.path();
    return f;
}

// the (aa, aa, distance, qi) list of every query; a whole-structure query on the device forms (nothing else is left to do per pair) in eight parts
static void qm_observed_lists(const qm_request &R, const qm_pairs &P, const qm_feat &F, const qm_form &form, qm_work &W) {
    W.aads.resize(R.n_queries);
    for (uint64_t t = 0; t < R.n_queries; ++t) {
        const bool parts = form.dev_expand && P.off[t + 1] - P.off[t] >= QM_PARTS_MIN;      // (small_par asks the system for its CPUs: only where it is used)
        qm_observed_list(F, P.pi.data(), P.off[t], P.off[t + 1], R.r0(t), parts ? &R.c->host_pool : nullptr, parts ? R.c->small_par(8) : 1u, W.aads[t]);
    }
}

// device expansion: the candidates are implied by the valid pairs
static void qm_implied_candidates(const qm_request &R, const qm_pairs &P, const qm_feat &F, const qm_form &form, qm_work &W) {
    const uint64_t np = P.pi.size();
    W.vpairs.reserve(form.valid_off[R.n_queries]);
    for (uint64_t k = 0; k < np; ++k) if (F.valid[k]) W.vpairs.push_back((uint32_t)k);
    W.cand_off.resize(R.n_queries + 1);
    for (uint64_t t = 0; t <= R.n_queries; ++t) W.cand_off[t] = form.valid_off[t] * form.per_pair;
    W.nc = W.cand_off[R.n_queries];
}
// host expansion: containers and records of every candidate (48 + 16 bytes each; reserved for the case without substitutions)
static void qm_host_candidates(const qm_request &R, const qm_pairs &P, const qm_feat &F, const qm_form &form, qm_work &W) {
    const uint64_t n_plain = form.valid_off[R.n_queries] * form.per_pair;
    W.cands.vf.reserve(n_plain * FD_QF); W.cands.c.reserve(n_plain);
    const qm_fields fl = qm_fields_of(R.p->hash_type);
    W.cand_off.assign(R.n_queries + 1, 0);
    for (uint64_t t = 0; t < R.n_queries; ++t) {
        const uint64_t a = R.q_off[t];
        qm_expand_query(F, P.pi.data(), P.pj.data(), P.off[t], P.off[t + 1], R.r0(t), R.q_index + a, R.q_off[t + 1] - a, R.any_subs ? R.subs + a : nullptr,
                        R.any_subs ? R.n_subs + a : nullptr, fl, R.thresholds(), W.cands);
        W.cand_off[t + 1] = W.cands.c.size();
    }
    W.nc = W.cands.c.size();
}

// ---- candidates -> hashes, one function per form
// host expansion: the containers go up, the hashes come back — once per bin configuration.  --multiple-bins: every candidate is inserted under
// every bin pair, in list order (insert_binned_hash, query.rs:59-70); the observed hash idf is looked up for stays the single-configuration one
// (query.rs:283-288)
static int qm_hash_host_form(const qm_request &R, const qm_work &W, qm_hashed &H) {
    int rc = hash_features_q(R.c, W.cands.vf.data(), W.nc, fd_make_consts(R.p).q, H.hashes.data(), FD_QF);
    H.cfg.resize(R.n_cfg);
    for (uint32_t k = 0; k < R.n_cfg && !rc; ++k) {
        H.cfg[k].resize(std::max<uint64_t>(W.nc, 1));
        rc = hash_features_q(R.c, W.cands.vf.data(), W.nc, fd_make_consts_cfg(R.p, k).q, H.cfg[k].data(), FD_QF);
    }
    return rc;
}
static qm_expand_par qm_device_par(const qm_request &R, const qm_form &form) {
    const qm_fields fl = qm_fields_of(R.p->hash_type);
    qm_expand_par P;
    memset(&P, 0, sizeof P);
    for (int z = 0; z < fl.ndi; ++z) P.di[z] = fl.di[z];
    for (int z = 0; z < fl.nai; ++z) P.ai[z] = fl.ai[z];
    P.ndi = fl.ndi; P.nai = fl.nai; P.n_dist = (uint32_t)R.n_dist; P.n_angle = (uint32_t)R.n_angle; P.per_pair = (uint32_t)form.per_pair;
    for (uint64_t z = 0; z < R.n_dist; ++z) P.dthr[z] = R.dist_thr[z];
    for (uint64_t z = 0; z < R.n_angle; ++z) P.athr[z] = R.athr[z];
    return P;
}
// The chain's outputs: ONE block of 25 bytes per candidate — [len u64 | kidx i64 | hash u32 | nseg u32 | first u8] x nc — on the device and, laid out
// the same, in the landing block, so that they come home in one copy launch (they were five)
struct qm_chain_block {
    uint64_t nc;
    size_t o_kidx() const { return nc * 8; }
    size_t o_hash() const { return nc * 16; }
    size_t o_nseg() const { return nc * 20; }
    size_t o_first() const { return nc * 24; }
    size_t bytes() const { return nc * 25; }
    uint64_t *len(uint8_t *b) const { return (uint64_t *)b; }
    long long *kidx(uint8_t *b) const { return (long long *)(b + o_kidx()); }
    uint32_t *hash(uint8_t *b) const { return (uint32_t *)(b + o_hash()); }
    uint32_t *nseg(uint8_t *b) const { return (uint32_t *)(b + o_nseg()); }
    uint8_t *first(uint8_t *b) const { return b + o_first(); }
};
// a motif batch: expansion + hashes -> per-query first-insertion dedupe (k_qm_dedupe) -> posting lengths, segment counts and list positions of
// EVERY candidate's hash (the index's length table; 17 k lookups per 128 queries) — three kernels back to back, one landing block, one wait; the
// host neither dedupes nor makes a second round trip for the lengths.  Without the chain's preconditions: hashes only.
// ws[WS_MISC2] still holds the pairs' containers (pair_features12)
static int qm_hash_chain_form(const qm_request &R, const qm_form &form, const qm_work &W, qm_hashed &H) {
    fdgpu_ctx *c = R.c;
    hipStream_t st = c->stream;
    const uint64_t nv = W.vpairs.size(), nc = W.nc, nq = R.n_queries;
    const qm_chain_block B = {nc};
    const size_t up_words = nv + 2 * (nq + 1) + 2, o_off = (nv + 1) & ~(size_t)1;      // upload: [valid pairs | cand_off, 8-byte aligned]
    uint32_t *up = (uint32_t *)c->host_pinned(FD_HP_UP, up_words * 4);
    std::vector<uint32_t> up_v;
    if (!up) { up_v.resize(up_words); up = up_v.data(); }
    memcpy(up, W.vpairs.data(), nv * 4);
    memcpy(up + o_off, W.cand_off.data(), (nq + 1) * 8);
    HIPCHK(c, c->ws[WS_MISC0].ensure(up_words * 4));
    HIPCHK(c, c->ws[WS_MISC1].ensure(B.bytes() + 64));
    uint32_t *d_up = c->ws[WS_MISC0].as<uint32_t>();
    uint8_t *d_blk = c->ws[WS_MISC1].as<uint8_t>();
    HIPCHK(c, hipMemcpyAsync(d_up, up, up_words * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_qm_expand_hash, dim3((unsigned)((nv + 63) / 64)), dim3(64), 0, st, c->ws[WS_MISC2].as<float>(), d_up, (uint32_t)nv, qm_device_par(R, form),
                       fd_make_consts(R.p).q, B.hash(d_blk));
    if (form.chain) hipLaunchKernelGGL(k_qm_dedupe, dim3((unsigned)nq), dim3(256), 0, st, B.hash(d_blk), (const uint64_t *)(d_up + o_off), B.first(d_blk));
    if (form.chain_len)
        fd_launch_posting_lookup(R.index->hashes, R.index->offsets, R.index->lens, R.index->n_hashes, B.hash(d_blk), nc, B.len(d_blk), B.nseg(d_blk), B.kidx(d_blk), st);
    HIPCHK(c, hipGetLastError());
    uint8_t *land = (uint8_t *)c->host_pinned(FD_HP_LAND, B.bytes() + 64);
    if (!land) { H.land_v.resize(B.bytes() + 64); land = H.land_v.data(); }
    // the whole block; without the lengths from the hashes on: hashes (and first-insertion flags; the segment counts between them are not read)
    const size_t from = form.chain_len ? 0 : B.o_hash(), to = form.chain ? B.bytes() : B.o_nseg();
    HIPCHK(c, hipMemcpyAsync(land + from, d_blk + from, to - from, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(H.hashes.data(), B.hash(land), nc * 4);
    if (form.chain) H.ch_first = B.first(land);
    if (form.chain_len) { H.ch_len = B.len(land); H.ch_kidx = B.kidx(land); H.ch_seg = B.nseg(land); }
    return FDGPU_OK;
}
// ONE large query (a whole-structure query): expansion, hashes and the first-insertion-wins dedupe on the device; only the hashes and the kept
// positions come back.  First insertion wins: stable sort of (hash, position) by hash, first of every run marked, marks compacted in position
// order.  The sort takes the build's key / id buffers
static int qm_hash_sort_form(const qm_request &R, const qm_form &form, const qm_work &W, qm_hashed &H) {
    fdgpu_ctx *c = R.c;
    hipStream_t st = c->stream;
    const uint64_t nv = W.vpairs.size(), nc = W.nc;
    HIPCHK(c, c->ws[WS_MISC0].ensure(nv * 4)); HIPCHK(c, c->ws[WS_MISC1].ensure(nc * 4));
    HIPCHK(c, c->ws[WS_KEYS_A].ensure(nc * 4)); HIPCHK(c, c->ws[WS_KEYS_B].ensure(nc * 4));
    HIPCHK(c, c->ws[WS_IDS_A].ensure(nc * 4)); HIPCHK(c, c->ws[WS_IDS_B].ensure(nc * 4));
    HIPCHK(c, c->ws[WS_GHIST].ensure((size_t)256 * std::max<uint32_t>(fd_rs_num_tiles(nc), 1) * 4));
    HIPCHK(c, c->ws[WS_TOT].ensure((256 + (size_t)(fd_rs_num_tiles(nc) / 128 + 2) * 256) * 8));
    HIPCHK(c, c->ws[WS_MISC4].ensure(nc + 8));
    HIPCHK(c, c->ws[WS_TILE_BO].ensure((nc + 2) * 8));
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(nc) * 8 + 64));
    HIPCHK(c, c->ws[WS_TOTAL].ensure(64));
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_MISC0].p, W.vpairs.data(), nv * 4, hipMemcpyHostToDevice, st));
    uint32_t *d_hash = c->ws[WS_MISC1].as<uint32_t>();
    hipLaunchKernelGGL(k_qm_expand_hash, dim3((unsigned)((nv + 63) / 64)), dim3(64), 0, st, c->ws[WS_MISC2].as<float>(), c->ws[WS_MISC0].as<uint32_t>(), (uint32_t)nv,
                       qm_device_par(R, form), fd_make_consts(R.p).q, d_hash);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(H.hashes.data(), d_hash, nc * 4, hipMemcpyDeviceToHost, st));
    uint32_t *ka = c->ws[WS_KEYS_A].as<uint32_t>(), *kb = c->ws[WS_KEYS_B].as<uint32_t>(), *va = c->ws[WS_IDS_A].as<uint32_t>(), *vb = c->ws[WS_IDS_B].as<uint32_t>();
    const unsigned gb = (unsigned)((nc + 255) / 256);
    HIPCHK(c, hipMemcpyAsync(ka, d_hash, nc * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_qm_iota, dim3(gb), dim3(256), 0, st, va, nc);
    const int cur = fd_radix_sort_pairs(ka, va, kb, vb, nc, 32, c->ws[WS_GHIST].as<uint32_t>(), c->ws[WS_TOT].as<uint64_t>(), st, nullptr);
    uint8_t *d_first = c->ws[WS_MISC4].as<uint8_t>();
    HIPCHK(c, hipMemsetAsync(d_first, 0, nc, st));
    hipLaunchKernelGGL(k_qm_first, dim3(gb), dim3(256), 0, st, cur ? kb : ka, cur ? vb : va, nc, d_first);
    fd_exclusive_scan<uint8_t>(d_first, nc, c->ws[WS_TILE_BO].as<uint64_t>(), c->ws[WS_SCANTMP].as<uint64_t>(), c->ws[WS_TOTAL].as<uint64_t>(), st);
    uint32_t *d_keep = cur ? ka : kb;      // the sort's other buffer is free again
    hipLaunchKernelGGL(k_qm_keep, dim3(gb), dim3(256), 0, st, d_first, c->ws[WS_TILE_BO].as<uint64_t>(), nc, d_keep);
    HIPCHK(c, hipGetLastError());
    uint64_t nk = 0;
    HIPCHK(c, hipMemcpyAsync(&nk, c->ws[WS_TOTAL].p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    H.dev_keep.resize(nk);
    // (a stray synchronous copy on the null stream into pageable memory, after the wait above: kept as it is)
    if (nk) HIPCHK(c, hipMemcpy(H.dev_keep.data(), d_keep, nk * 4, hipMemcpyDeviceToHost));
    return FDGPU_OK;
}
static int qm_hash_candidates(const qm_request &R, const qm_form &form, const qm_work &W, qm_hashed &H) {
    H.hashes.resize(std::max<uint64_t>(W.nc, 1));
    const int rc = !form.dev_expand ? qm_hash_host_form(R, W, H) : form.dev_dedupe ? qm_hash_sort_form(R, form, W, H) : qm_hash_chain_form(R, form, W, H);
    if (R.n_cfg) for (uint32_t k = 0; k < R.n_cfg; ++k) H.planes.push_back(H.cfg[k].data());
    else H.planes.push_back(H.hashes.data());
    return rc;
}

// first insertion wins (the reference's hash map keeps the entry a hash was first inserted with): the device's answer where a device form gave
// one, else per query on the host
static void qm_first_insertions(const qm_request &R, const qm_form &form, const qm_work &W, qm_hashed &H, qm_kept &K) {
    K.keeps.resize(R.n_queries);
    std::vector<uint64_t> tab;
    for (uint64_t t = 0; t < R.n_queries; ++t) {
        const qm_insertions I = H.insertions(W, t);
        std::vector<uint32_t> &keep = K.keeps[t];
        if (form.dev_dedupe) keep.swap(H.dev_keep);
        else if (H.ch_first) { keep.reserve((size_t)I.n_ins / 2 + 8); for (uint64_t pos = 0; pos < I.n_ins; ++pos) if (H.ch_first[I.c0 + pos]) keep.push_back((uint32_t)pos); }
        else qm_first_wins(I, tab, keep);
        K.n_keep += keep.size();
    }
}

// the observed candidate of every valid pair, in candidate order: its pair and its hash
struct qm_observed { std::vector<uint32_t> pair_v, hash; const uint32_t *pair = nullptr; };
static void qm_observed_candidates(const qm_form &form, const qm_work &W, const qm_hashed &H, qm_observed &O) {
    if (form.dev_expand) {
        O.pair = W.vpairs.data();
        O.hash.resize(W.vpairs.size());
        for (size_t v = 0; v < O.hash.size(); ++v) O.hash[v] = H.hashes[v * form.per_pair];
        return;
    }
    for (uint64_t z = 0; z < W.nc; ++z)
        if (W.cands.c[z].primary) { O.hash.push_back(H.hashes[z]); O.pair_v.push_back(W.cands.c[z].pair); }
    O.pair = O.pair_v.data();
}
// the chain looked every candidate up: pick the kept entries and the observed hashes
static void qm_lengths_from_chain(const qm_form &form, const qm_work &W, const qm_hashed &H, const qm_kept &K, qm_lengths &L) {
    size_t w = 0;
    for (size_t t = 0; t < K.keeps.size(); ++t)
        for (uint32_t pos : K.keeps[t]) { const uint64_t z = W.cand_off[t] + pos; L.ent_len[w] = H.ch_len[z]; L.ent_seg[w] = H.ch_seg[z]; L.ent_kidx[w] = H.ch_kidx[z]; ++w; }
    for (uint64_t v = 0; v < W.vpairs.size(); ++v, ++w) { const uint64_t z = v * form.per_pair; L.ent_len[w] = H.ch_len[z]; L.ent_seg[w] = H.ch_seg[z]; L.ent_kidx[w] = H.ch_kidx[z]; }
}
// ... or one lookup of the kept entries' hashes, then the observed ones; large requests stay in the page-locked block (read once, in place)
static int qm_lengths_lookup(const qm_request &R, const qm_work &W, const qm_hashed &H, const qm_kept &K, const qm_observed &O, qm_lengths &L) {
    std::vector<uint32_t> ph;
    ph.reserve(K.n_keep + O.hash.size());
    for (uint64_t t = 0; t < R.n_queries; ++t) {
        const qm_insertions I = H.insertions(W, t);
        for (uint32_t pos : K.keeps[t]) ph.push_back(qm_hash_at(I, pos));
    }
    ph.insert(ph.end(), O.hash.begin(), O.hash.end());
    const uint8_t *land = nullptr;
    const int rc = fd_posting_lengths_segs(R.c, R.index, ph.data(), ph.size(), L.ent_len.data(), L.ent_seg.data(), L.ent_kidx.data(), ph.size() >= QM_PARTS_MIN ? &land : nullptr);
    if (!rc && land) { L.e_len = (const uint64_t *)land; L.e_kidx = (const long long *)(land + ph.size() * 8); L.e_seg = (const uint32_t *)(land + ph.size() * 16); }
    return rc;
}
// ONE posting-length pass: the observed (primary) hash of every pair — idf = log2(S / len), query.rs:17-32 — and every entry that enters a map;
// the maps remember the latter (post_len / post_seg) so that scoring them needs no second pass over the same lists
static int qm_posting_lengths(const qm_request &R, const qm_pairs &P, const qm_form &form, const qm_work &W, const qm_hashed &H, const qm_kept &K, qm_lengths &L) {
    const size_t np = P.pi.size();
    L.pair_idf.assign(std::max<size_t>(np, 1), 0.0f); L.pair_primary.assign(std::max<size_t>(np, 1), 0u);
    qm_observed O;
    qm_observed_candidates(form, W, H, O);
    const size_t n_obs = O.hash.size(), n_ent = K.n_keep + n_obs;
    for (size_t v = 0; v < n_obs; ++v) L.pair_primary[O.pair[v]] = O.hash[v];
    if (!R.index) return FDGPU_OK;
    L.ent_len.assign(std::max<size_t>(n_ent, 1), 0); L.ent_seg.assign(std::max<size_t>(n_ent, 1), 0); L.ent_kidx.assign(std::max<size_t>(n_ent, 1), -1);
    L.e_len = L.ent_len.data(); L.e_seg = L.ent_seg.data(); L.e_kidx = L.ent_kidx.data();
    if (H.ch_len) qm_lengths_from_chain(form, W, H, K, L);
    else if (const int rc = qm_lengths_lookup(R, W, H, K, O, L)) return rc;
    // idf of the observed hash of every pair: log2f is ~8 ns a call — 0.7 ms for the 88 k pairs of a whole-structure query on one thread
    const uint64_t *len = L.e_len + K.n_keep;
    const float S = R.total_structures;
    const auto idf_part = [&](unsigned z) { for (size_t v = n_obs * z / 8; v < n_obs * (z + 1) / 8; ++v) L.pair_idf[O.pair[v]] = len[v] > 0 ? log2f(S / (float)len[v]) : 0.0f; };
    // (this loop sizes its helpers without small_par, so on a lane context it alone leaves the lane's thread; making it follow the other two
    // would change what a lane does and is left as it is)
    if (n_obs < QM_PARTS_MIN) for (unsigned z = 0; z < 8; ++z) idf_part(z);
    else qm_run_parts(&R.c->host_pool, std::min(8u, std::max(1u, std::thread::hardware_concurrency())), 8, idf_part);
    return FDGPU_OK;
}

// one block per map (a map was 15 allocations, a batch of 128 queries two thousand)
static int qm_assemble(const qm_request &R, const qm_pairs &P, const qm_form &form, const qm_work &W, const qm_hashed &H, const qm_kept &K, const qm_lengths &L) {
    uint64_t keep_at = 0;      // entries of the queries in front
    for (uint64_t t = 0; t < R.n_queries; ++t) {
        const std::vector<uint32_t> &keep = K.keeps[t];
        const qm_map_src S = {keep.data(), keep.size(), H.insertions(W, t), form.dev_expand ? nullptr : W.cands.c.data(), W.vpairs.data(), form.per_pair, P.pi.data(),
                              P.pj.data(), R.r0(t), L.pair_idf.data(), L.pair_primary.data(), L.e_len ? L.e_len + keep_at : nullptr, L.e_seg ? L.e_seg + keep_at : nullptr,
                              L.e_kidx ? L.e_kidx + keep_at : nullptr, R.index ? R.index->uid : 0, R.q_index + R.q_off[t], (size_t)(R.q_off[t + 1] - R.q_off[t]), &W.aads[t]};
        fd_query_map *m = qm_fill_map(S, &R.c->host_pool, form.dev_expand && keep.size() >= QM_PARTS_MIN ? R.c->small_par(8) : 1u);
        if (!m) { for (uint64_t u = 0; u < t; ++u) { fdgpu_query_map_free(R.out[u]); R.out[u] = nullptr; } return FDGPU_ENOMEM; }
        R.out[t] = m;
        keep_at += keep.size();
    }
    return FDGPU_OK;
}

// make_query_map (src/controller/query.rs:208-329) for MANY queries with three launches in total (pair features, hashes of
// the expanded candidates, posting lengths of the primary hashes): query t is structure q_struct[t] of qb with the residues
// q_index[q_off[t] .. q_off[t+1]); subs / n_subs run parallel to q_index.  out[t] is released with fdgpu_query_map_free.
extern "C" int fdgpu_make_query_map_batch(fdgpu_ctx *c, const fdgpu_batch *qb, uint64_t n_queries, const uint32_t *q_struct, const uint64_t *q_off,
                                          const uint32_t *q_index, const uint8_t *const *subs, const uint32_t *n_subs, const float *dist_thr,
                                          uint64_t n_dist, const float *angle_thr_deg, uint64_t n_angle, const fd_hash_params *p,
                                          const fdgpu_index *index, float total_structures, fd_query_map **out) { FD_LOCK(c);
    qm_request R = {c, qb, n_queries, q_struct, q_off, q_index, subs, n_subs, dist_thr, n_dist, angle_thr_deg, n_angle, p, index, total_structures, out};
    int rc = qm_read_request(R);
    if (rc) return rc;
    qm_pairs P;
    qm_list_pairs(n_queries, q_struct, q_off, q_index, qb->h_res_off.data(), P);
    if (R.trace) fprintf(stderr, "[fdgpu_query_map] pairs listed at %.3f ms\n", R.ms());
    qm_feat_store FS;
    qm_feat F;
    if ((rc = qm_pair_features(R, P, FS, F))) return rc;
    if (R.trace) fprintf(stderr, "[fdgpu_query_map] %llu pairs: features at %.3f ms\n", (unsigned long long)P.pi.size(), R.ms());
    const qm_form form = qm_choose_form(R, P, F);
    qm_work W;
    qm_observed_lists(R, P, F, form, W);
    if (form.dev_expand) qm_implied_candidates(R, P, F, form, W);
    else qm_host_candidates(R, P, F, form, W);
    if (R.trace) fprintf(stderr, "[fdgpu_query_map] %llu candidates expanded at %.3f ms\n", (unsigned long long)W.nc, R.ms());
    qm_hashed H;
    if ((rc = qm_hash_candidates(R, form, W, H))) return rc;
    if (R.trace) fprintf(stderr, "[fdgpu_query_map] hashed at %.3f ms\n", R.ms());
    qm_kept K;
    qm_first_insertions(R, form, W, H, K);
    if (R.trace) fprintf(stderr, "[fdgpu_query_map] first insertions at %.3f ms\n", R.ms());
    qm_lengths L;
    if ((rc = qm_posting_lengths(R, P, form, W, H, K, L))) return rc;
    if (R.trace) fprintf(stderr, "[fdgpu_query_map] posting lengths at %.3f ms\n", R.ms());
    if ((rc = qm_assemble(R, P, form, W, H, K, L))) return rc;
    if (R.trace) fprintf(stderr, "[fdgpu_query_map] maps built at %.3f ms\n", R.ms());
    return FDGPU_OK;
}

// one query = structure 0 of qb
extern "C" int fdgpu_make_query_map(fdgpu_ctx *c, const fdgpu_batch *qb, const uint32_t *q_index, uint64_t n_q, const uint8_t *const *subs,
                                    const uint32_t *n_subs, const float *dist_thr, uint64_t n_dist, const float *angle_thr_deg, uint64_t n_angle,
                                    const fd_hash_params *p, const fdgpu_index *index, float total_structures, fd_query_map **out) { FD_LOCK(c);
    if (!c || !qb || !p || !out || qb->n_struct < 1 || (n_q && !q_index)) return FDGPU_EINVAL;
    const uint32_t s0 = 0;
    const uint64_t off[2] = {0, n_q};
    return fdgpu_make_query_map_batch(c, qb, 1, &s0, off, q_index, subs, n_subs, dist_thr, n_dist, angle_thr_deg, n_angle, p, index, total_structures, out);
}

extern "C" int fdgpu_debug_last_query_map_path(fdgpu_ctx *c, uint32_t *flags) { FD_LOCK(c);
    if (!c || !flags) return FDGPU_EINVAL;
    *flags = c->last_query_map_path;
    return FDGPU_OK;
}
