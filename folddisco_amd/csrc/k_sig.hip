// k_sig.hip — index signatures (fdgpu_index_signatures), their all-pairs compare (fdgpu_signature_pairs), their k nearest neighbours
// (fdgpu_signature_neighbors) and their greedy clusters (fdgpu_signature_clusters, described at its kernels below); the definitions are
// include/fdgpu.h and fd_signature.h, the host forms fd_signatures_host.cpp.
//
// Signatures: the index is walked in windows of structures.  Per window the device stage of the rows (fd_rows_device, k_rows.hip) leaves the
// window's hashes in (id, hash) order and the row offsets in the context's workspaces, and
//   k_sg_reduce   wavefront per row: the lanes stride the row's hashes (val[row_off[s] + lane + 64 i], coalesced), each mixes its hash once,
//                 keeps its share of the sum and the xor in registers and folds the bucket minimum into the wavefront's own 64 words of LDS
//                 (atomicMin on LDS; no global atomic).  A wave reduction of sum and xor, then the 70 words of the record leave in two
//                 wave-wide stores.  Sums, xors and minima do not depend on an order, so the table is the same from run to run.
// Rows are uneven (0 to more than 10^5 hashes); every row keeps one wavefront, no workgroup class for the long ones.
// The window's table is copied to its place in the page-locked result behind the kernel, in stream order, so the next window may reuse it.
// Byte work per window, beyond the rows' stages: 4 bytes per posting and 16 per structure read, 280 per structure written and copied out.
//
// Pairs: both tables are uploaded (self mode: one), and
//   k_sg_match    256-thread workgroup: every lane owns one signature of B in registers (64 words + the mask of its empty buckets); the
//                 workgroup stages tiles of 64 signatures of A in LDS (sk 16 KB, the six header words, a 64-bit empty mask each) and every lane
//                 compares its signature with the tile's, one signature of A per step — the LDS address is the same for the whole wavefront, a
//                 broadcast read.  Per pair 64 compares and adds and one popcount.  A wavefront's qualifying pairs of a step take their slots
//                 from the one global cursor with ONE atomicAdd; a record is written only below max_pairs, the cursor counts on, so the true
//                 count comes back.  Self mode skips the tiles wholly on or below the diagonal and tests a < b inside the others.
// The records are sorted by (a, b) on the host (at most max_pairs of them), so the result does not depend on the order the kernel found them in.
// VALU work: 128 lane-operations per pair.  Workspace: 280 bytes per signature, 12 per pair slot (at most min(max_pairs, every pair)).
//
// Neighbours: the tables are uploaded as for the pairs, and
//   k_sg_near        the layout of k_sg_match (a query per lane in registers, tiles of 64 candidates broadcast from LDS, gridDim.y shares the
//                    tiles), with a selection in place of the cursor: every lane keeps its k nearest so far as a sorted list in LDS
//                    ([slot][lane], k * 1.5 KB per workgroup, sized by the launch) and the list's last entry in registers.  A candidate that
//                    passes the predicate is compared with that entry first; only a winner touches the list (a bisection and a shift: about
//                    k ln(nD / k) of them per query, none in the steady state).  No global atomic, no cursor.  Every tile in self mode too.
//   k_sg_near_merge  only when gridDim.y > 1: a wavefront per query takes the nearest head of the gridDim.y sorted lists k times.
// The order (fd_sig_nearer) is total, so the result is the same bytes for every split.  Workspace: 280 bytes per signature, 8 k per query and split.
#include <algorithm>
#include <cstring>
#include "fdgpu_internal.h"
#include "fd_api_common.h"
#include "fd_postings.h"
#include "fd_signature.h"

#define SG_WINDOW_DEFAULT 16384u
#define SG_TILE_A 64u           // signatures of A per tile
#define SG_BLOCK_B 256u         // signatures of B per workgroup: one per lane

__device__ __forceinline__ uint64_t sg_wave_sum64(uint64_t v) {
    for (int o = FD_WAVE / 2; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, FD_WAVE);
    return v;
}
__device__ __forceinline__ uint64_t sg_wave_xor64(uint64_t v) {
    for (int o = FD_WAVE / 2; o > 0; o >>= 1) v ^= (uint64_t)__shfl_xor((unsigned long long)v, o, FD_WAVE);
    return v;
}

// ---- reduce: wavefront per row s = 0 .. W - 1.  Reads val[row_off[s] .. row_off[s + 1]) (k_rw_bounds: offsets ascend and end at n), writes the
// 70 words of record s.  A wavefront's table is its own: the LDS unit takes one wavefront's operations in their order, no workgroup barrier
__global__ __launch_bounds__(256) void k_sg_reduce(const uint32_t *__restrict__ val, const uint64_t *__restrict__ row_off, uint64_t W, uint32_t *__restrict__ out) {
    __shared__ uint32_t mins[4][64];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t s = (uint64_t)blockIdx.x * 4u + wv;
    if (s >= W) return;
    uint32_t *mine = mins[wv];
    mine[lane] = FD_SIG_EMPTY;
    __builtin_amdgcn_wave_barrier();
    const uint64_t r0 = row_off[s], r1 = row_off[s + 1];
    uint64_t d0 = 0, d1 = 0;
    for (uint64_t i = r0 + lane; i < r1; i += FD_WAVE) {
        const uint64_t m = fd_sig_mix(val[i]);
        d0 += m; d1 ^= m;
        atomicMin(&mine[fd_sig_bucket(m)], fd_sig_value(m));
    }
    d0 = sg_wave_sum64(d0); d1 = sg_wave_xor64(d1);
    __builtin_amdgcn_wave_barrier();
    const uint32_t sk_lo = mine[lane >= 6u ? lane - 6u : 0u], sk_hi = mine[lane < 6u ? 58u + lane : 0u];
    const uint32_t head[6] = {(uint32_t)(r1 - r0), 0u, (uint32_t)d0, (uint32_t)(d0 >> 32), (uint32_t)d1, (uint32_t)(d1 >> 32)};
    uint32_t hw = head[0];
#pragma unroll
    for (uint32_t k = 1; k < 6; ++k) if (lane == k) hw = head[k];
    uint32_t *rec = out + s * FD_SIG_WORDS;
    rec[lane] = lane < 6u ? hw : sk_lo;               // words 0 .. 63
    if (lane < 6u) rec[64u + lane] = sk_hi;           // words 64 .. 69
}

static int signatures_impl(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t id_lo, uint64_t id_hi, uint64_t window, fd_signature **out) {
    reset_timings(c);
    hipStream_t st = c->stream;
    const uint64_t N = id_hi - id_lo;
    if (!window) window = SG_WINDOW_DEFAULT;
    fd_signature *res = (fd_signature *)fd_out_alloc(std::max<uint64_t>(N, 1) * sizeof(fd_signature), true);
    if (!res) FAIL(c, FDGPU_ENOMEM, "index signatures: out of host memory");
    int rc = FDGPU_OK;
    hipError_t e = hipSuccess;
    for (uint64_t lo = id_lo; lo < id_hi && rc == FDGPU_OK && e == hipSuccess; lo += std::min<uint64_t>(window, id_hi - lo)) {
        const uint64_t W = std::min<uint64_t>(window, id_hi - lo);
        fd_rows_dev R;
        rc = fd_rows_device(c, ix, lo, lo + W, "index signatures", &R);
        if (rc != FDGPU_OK) break;
        e = c->ws[WS_SG_TAB].ensure(W * sizeof(fd_signature));
        if (e != hipSuccess) break;
        uint32_t *tab = c->ws[WS_SG_TAB].as<uint32_t>();
        {
            StageTimer t(c, "sig_reduce", R.n * 4 + (W + 1) * 8 + W * sizeof(fd_signature));
            hipLaunchKernelGGL(k_sg_reduce, dim3(fd_grid(W, 4)), dim3(256), 0, st, R.val, R.row_off, W, tab);
        }
        e = hipGetLastError();
        if (e != hipSuccess) break;
        {
            StageTimer t(c, "sig_copy", W * sizeof(fd_signature));
            e = hipMemcpyAsync(res + (lo - id_lo), tab, W * sizeof(fd_signature), hipMemcpyDeviceToHost, st);
        }
    }
    if (rc == FDGPU_OK && e == hipSuccess) e = hipStreamSynchronize(st);      // the result is complete, and the workspaces free again, when the call returns
    if (rc != FDGPU_OK || e != hipSuccess) {
        (void)hipStreamSynchronize(st);                                       // nothing of a failed call still writes into the block
        fdgpu_free(res);
        if (rc != FDGPU_OK) return rc;
        c->err = std::string("index signatures: ") + hipGetErrorString(e);
        return FDGPU_EHIP;
    }
    *out = res;
    return FDGPU_OK;
}

extern "C" int fdgpu_index_signatures(fdgpu_ctx *c, const fdgpu_index *ix, uint64_t id_lo, uint64_t id_hi, uint64_t window, fd_signature **out) { FD_LOCK(c);
    if (!c || !ix || !out) return FDGPU_EINVAL;
    *out = nullptr;
    if (id_lo < ix->first_id || id_lo > id_hi || id_hi > ix->first_id + ix->n_structures)
        FAIL(c, FDGPU_EINVAL, "index signatures: the range is not inside [first_id, first_id + n_structures]");
    return signatures_impl(c, ix, id_lo, id_hi, window, out);
}

// ---- match.  Grid: x = workgroups of 256 signatures of B, y = the tiles of A a workgroup takes in turn (tile ta = blockIdx.y, + gridDim.y, ...).
// Reads A[0 .. nA), B[0 .. nB); writes pairs[slot] for slot < max_pairs only.
// the tile A[a0 .. a0 + 64) into LDS for the whole workgroup of 256 (k_sg_match, k_sg_near): sketches, header words, a mask of the empty buckets each
__device__ __forceinline__ void sg_stage_tile(const uint32_t *__restrict__ A, uint32_t nA, uint64_t a0, uint32_t (*a_sk)[64], uint32_t (*a_head)[6],
                                              unsigned long long *a_empty) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    __syncthreads();                                // the tile before is read to its end
    const uint32_t n_in = (uint32_t)std::min<uint64_t>(SG_TILE_A, nA - a0);
    for (uint32_t w = threadIdx.x; w < SG_TILE_A * FD_SIG_WORDS; w += 256u) {
        const uint32_t i = w / FD_SIG_WORDS, f = w % FD_SIG_WORDS;
        const uint32_t x = i < n_in ? A[a0 * FD_SIG_WORDS + w] : (f == 0 ? 0u : FD_SIG_EMPTY);      // beyond the table: n = 0, never reported
        if (f < 6) a_head[i][f] = x; else a_sk[i][f - 6] = x;
    }
    __syncthreads();
    for (uint32_t i = wv * 16u; i < wv * 16u + 16u; ++i) {      // the empty masks, a wavefront per 16 signatures
        const unsigned long long em = __ballot(a_sk[i][lane] == FD_SIG_EMPTY);
        if (lane == 0) a_empty[i] = em;
    }
    __syncthreads();
}

struct sg_match_args { const uint32_t *A; const uint32_t *B; uint32_t nA, nB, thr64, self; fd_sig_pair *pairs; unsigned long long *cursor; unsigned long long max_pairs; };

__global__ __launch_bounds__(256) void k_sg_match(sg_match_args P) {
    __shared__ uint32_t a_sk[SG_TILE_A][64];
    __shared__ uint32_t a_head[SG_TILE_A][6];
    __shared__ unsigned long long a_empty[SG_TILE_A];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t j = (uint64_t)blockIdx.x * SG_BLOCK_B + threadIdx.x;      // the lane's signature of B
    const bool have = j < P.nB;
    uint32_t b[64];
    uint32_t bn = 0, bd0l = 0, bd0h = 0, bd1l = 0, bd1h = 0;
    unsigned long long b_empty = 0;
    {
        const uint32_t *pb = P.B + (have ? j : 0) * FD_SIG_WORDS;
        if (have) { bn = pb[0]; bd0l = pb[2]; bd0h = pb[3]; bd1l = pb[4]; bd1h = pb[5]; }
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k) {
            b[k] = have ? pb[6 + k] : FD_SIG_EMPTY;
            b_empty |= (unsigned long long)(b[k] == FD_SIG_EMPTY ? 1u : 0u) << k;
        }
    }
    const uint32_t tiles = (P.nA + SG_TILE_A - 1) / SG_TILE_A;
    const uint64_t b_last = std::min<uint64_t>((uint64_t)blockIdx.x * SG_BLOCK_B + SG_BLOCK_B, P.nB) - 1;      // the workgroup's last signature of B
    for (uint32_t ta = blockIdx.y; ta < tiles; ta += gridDim.y) {
        const uint64_t a0 = (uint64_t)ta * SG_TILE_A;
        if (P.self && a0 >= b_last) continue;           // no a < b in this tile (the same for the whole workgroup)
        sg_stage_tile(P.A, P.nA, a0, a_sk, a_head, a_empty);
        for (uint32_t i = 0; i < SG_TILE_A; ++i) {
            uint32_t eq = 0;
#pragma unroll
            for (uint32_t k = 0; k < 64; ++k) eq += a_sk[i][k] == b[k] ? 1u : 0u;
            const uint32_t E = (uint32_t)__popcll(a_empty[i] & b_empty);
            const uint64_t a = a0 + i;
            const bool ok = have && fd_sig_reported(a_head[i][0], bn, eq, E, P.thr64) && (!P.self || a < j);
            const unsigned long long vote = __ballot(ok);
            if (vote) {                                 // one atomic for the wavefront's pairs of this step
                unsigned long long base = 0;
                const uint32_t leader = (uint32_t)__ffsll((long long)vote) - 1u;
                if (lane == leader) base = atomicAdd(P.cursor, (unsigned long long)__popcll(vote));
                base = __shfl(base, (int)leader, FD_WAVE);
                const unsigned long long slot = base + (unsigned long long)__popcll(vote & ((1ull << lane) - 1ull));
                if (ok && slot < P.max_pairs) {
                    const bool same = a_head[i][0] == bn && a_head[i][2] == bd0l && a_head[i][3] == bd0h && a_head[i][4] == bd1l && a_head[i][5] == bd1h;
                    fd_sig_pair r;
                    r.a = (uint32_t)a; r.b = (uint32_t)j; r.match = (uint8_t)(eq - E); r.filled = (uint8_t)(64u - E); r.flags = same ? FD_SIG_IDENTICAL : 0u;
                    P.pairs[slot] = r;
                }
            }
        }
    }
}

static int pairs_impl(fdgpu_ctx *c, const fd_signature *A, uint64_t nA, const fd_signature *B, uint64_t nB, uint32_t thr64, uint64_t max_pairs,
                      fd_sig_pair **pairs, uint64_t *n_pairs) {
    reset_timings(c);
    hipStream_t st = c->stream;
    const bool self = B == nullptr;
    if (self) nB = nA;
    unsigned long long found = 0;
    // every pair there is: the slots never need to be more
    const long double all = self ? (long double)nA * (long double)(nA ? nA - 1 : 0) / 2 : (long double)nA * (long double)nB;
    const uint64_t cap = all < (long double)max_pairs ? (uint64_t)all : max_pairs;
    if (nA && nB) {
        HIPCHK(c, c->ws[WS_SG_TAB].ensure(nA * sizeof(fd_signature)));
        if (!self) HIPCHK(c, c->ws[WS_SG_TAB_B].ensure(nB * sizeof(fd_signature)));
        HIPCHK(c, c->ws[WS_SG_PAIRS].ensure(std::max<uint64_t>(cap, 1) * sizeof(fd_sig_pair)));
        HIPCHK(c, c->ws[WS_SG_CURSOR].ensure(64));
        uint32_t *dA = c->ws[WS_SG_TAB].as<uint32_t>(), *dB = self ? dA : c->ws[WS_SG_TAB_B].as<uint32_t>();
        unsigned long long *cursor = c->ws[WS_SG_CURSOR].as<unsigned long long>();
        {
            StageTimer t(c, "sigpairs_upload", (nA + (self ? 0 : nB)) * sizeof(fd_signature));
            HIPCHK(c, hipMemcpyAsync(dA, A, nA * sizeof(fd_signature), hipMemcpyHostToDevice, st));
            if (!self) HIPCHK(c, hipMemcpyAsync(dB, B, nB * sizeof(fd_signature), hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemsetAsync(cursor, 0, 8, st));
        }
        const uint32_t blocks_b = fd_grid(nB, SG_BLOCK_B), tiles = fd_grid(nA, SG_TILE_A);
        // a workgroup loads its signatures of B once and walks its share of the tiles: enough workgroups to fill the device, no more
        const uint32_t gy = std::max<uint32_t>(1u, std::min<uint32_t>(std::min<uint32_t>(tiles, 65535u), fd_grid(4096, blocks_b)));
        {
            StageTimer t(c, "sigpairs_match", (uint64_t)blocks_b * ((uint64_t)SG_BLOCK_B + (uint64_t)(tiles / gy + 1) * SG_TILE_A) * gy * sizeof(fd_signature));
            const sg_match_args P{dA, dB, (uint32_t)nA, (uint32_t)nB, thr64, self ? 1u : 0u, c->ws[WS_SG_PAIRS].as<fd_sig_pair>(), cursor, cap};
            hipLaunchKernelGGL(k_sg_match, dim3(blocks_b, gy), dim3(256), 0, st, P);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&found, cursor, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    *n_pairs = found;
    if (found > max_pairs) FAIL(c, FDGPU_ERANGE, "signature pairs: " + std::to_string(found) + " pairs qualify, more than max_pairs = " + std::to_string(max_pairs));
    fd_sig_pair *res = (fd_sig_pair *)fd_out_alloc(std::max<uint64_t>(found, 1) * sizeof(fd_sig_pair));
    if (!res) FAIL(c, FDGPU_ENOMEM, "signature pairs: out of host memory");
    if (found) {
        hipError_t e;
        {
            StageTimer t(c, "sigpairs_copy", found * sizeof(fd_sig_pair));
            e = fd_d2h_big(c, res, c->ws[WS_SG_PAIRS].p, found * sizeof(fd_sig_pair));
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { fdgpu_free(res); c->err = std::string("signature pairs: ") + hipGetErrorString(e); return FDGPU_EHIP; }
        std::sort(res, res + found, [](const fd_sig_pair &x, const fd_sig_pair &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    }
    *pairs = res;
    return FDGPU_OK;
}

extern "C" int fdgpu_signature_pairs(fdgpu_ctx *c, const fd_signature *A, uint64_t nA, const fd_signature *B, uint64_t nB, uint32_t thr64, uint64_t max_pairs,
                                     fd_sig_pair **pairs, uint64_t *n_pairs) { FD_LOCK(c);
    if (!c || !pairs || !n_pairs) return FDGPU_EINVAL;
    *pairs = nullptr; *n_pairs = 0;
    if (thr64 < 1 || thr64 > 64) FAIL(c, FDGPU_EINVAL, "signature pairs: thr64 must be 1 .. 64");
    if (nA > 0xffffffffull || (B && nB > 0xffffffffull)) FAIL(c, FDGPU_EINVAL, "signature pairs: a table of 2^32 or more signatures");
    if (nA && !A) FAIL(c, FDGPU_EINVAL, "signature pairs: table A is NULL");
    const int rc = pairs_impl(c, A, nA, B, nB, thr64, max_pairs, pairs, n_pairs);
    if (rc != FDGPU_OK) (void)hipStreamSynchronize(c->stream);
    return rc;
}

// ---- neighbours.  Grid as k_sg_match: x = workgroups of 256 queries (one per lane), y = the tiles of D a workgroup takes in turn.  Reads
// Q[0 .. nQ), D[0 .. nD), excl[0 .. nQ) if given; writes out[(blockIdx.y * nQ + q) * k + 0 .. k) for its queries q < nQ: the lane's k nearest among
// the tiles it saw, nearest first, empty slots behind them.  Dynamic LDS: k * 1536 bytes, the lists as [slot][lane]: a word for the id and a
// halfword for match | filled << 7 | identical << 14 (six bytes a slot: k = 32 leaves room for two workgroups per CU), the lanes of a wavefront
// on different banks whatever slot each of them is at.
struct sg_near_args { const uint32_t *Q; const uint32_t *D; const uint32_t *excl; uint32_t nQ, nD, thr64, self, k; uint2 *out; };
#define SG_NB_LDS_PER_K (SG_BLOCK_B * 6u)

// y as the second word of a fd_sig_neighbor: match | filled << 8 | flags << 16
__device__ __forceinline__ bool sg_nearer_packed(uint32_t m, uint32_t f, uint32_t id, uint32_t mf, uint32_t id_y) {
    return fd_sig_nearer(m, f, id, mf & 0xffu, (mf >> 8) & 0xffu, id_y);
}
__device__ __forceinline__ uint32_t sg_mf_word(uint32_t h) { return (h & 0x7fu) | ((h >> 7) & 0x7fu) << 8 | (h >> 14) << 16; }      // the LDS halfword -> that word

__global__ __launch_bounds__(256) void k_sg_near(sg_near_args P) {
    __shared__ uint32_t a_sk[SG_TILE_A][64];
    __shared__ uint32_t a_head[SG_TILE_A][6];
    __shared__ unsigned long long a_empty[SG_TILE_A];
    extern __shared__ uint32_t nb_lds[];
    const uint32_t t = threadIdx.x, K = P.k;
    uint32_t *nb_id = nb_lds + t;                                             // slot s at [s * 256]
    uint16_t *nb_mf = reinterpret_cast<uint16_t *>(nb_lds + K * SG_BLOCK_B) + t;
    const uint64_t j = (uint64_t)blockIdx.x * SG_BLOCK_B + t;                 // the lane's query
    const bool have = j < P.nQ;
    uint32_t b[64];
    uint32_t bn = 0, bd0l = 0, bd0h = 0, bd1l = 0, bd1h = 0;
    unsigned long long b_empty = 0;
    {
        const uint32_t *pb = P.Q + (have ? j : 0) * FD_SIG_WORDS;
        if (have) { bn = pb[0]; bd0l = pb[2]; bd0h = pb[3]; bd1l = pb[4]; bd1h = pb[5]; }
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k) {
            b[k] = have ? pb[6 + k] : FD_SIG_EMPTY;
            b_empty |= (unsigned long long)(b[k] == FD_SIG_EMPTY ? 1u : 0u) << k;
        }
    }
    const uint32_t skip = P.self ? (uint32_t)j : (P.excl && have ? P.excl[j] : FD_SIG_NO_ID);
    for (uint32_t s = 0; s < K; ++s) { nb_id[s * SG_BLOCK_B] = FD_SIG_NO_ID; nb_mf[s * SG_BLOCK_B] = 0u; }
    uint32_t kth_id = FD_SIG_NO_ID, kth_mf = 0u;       // the list's last slot: what a candidate has to beat
    const uint32_t tiles = (P.nD + SG_TILE_A - 1) / SG_TILE_A;
    for (uint32_t ta = blockIdx.y; ta < tiles; ta += gridDim.y) {
        const uint64_t a0 = (uint64_t)ta * SG_TILE_A;
        sg_stage_tile(P.D, P.nD, a0, a_sk, a_head, a_empty);
        for (uint32_t i = 0; i < SG_TILE_A; ++i) {
            uint32_t eq = 0;
#pragma unroll
            for (uint32_t k = 0; k < 64; ++k) eq += a_sk[i][k] == b[k] ? 1u : 0u;
            const uint32_t E = (uint32_t)__popcll(a_empty[i] & b_empty);
            const uint32_t a = (uint32_t)(a0 + i), m = eq - E, f = 64u - E;
            // a lane without a query and a slot beyond the table have n = 0: never a candidate
            if (fd_sig_reported(bn, a_head[i][0], eq, E, P.thr64) && a != skip && sg_nearer_packed(m, f, a, kth_mf, kth_id)) {
                const bool same = a_head[i][0] == bn && a_head[i][2] == bd0l && a_head[i][3] == bd0h && a_head[i][4] == bd1l && a_head[i][5] == bd1h;
                uint32_t lo = 0, hi = K - 1;           // its slot: the first one it is nearer than (the last one at the latest), by bisection
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (sg_nearer_packed(m, f, a, sg_mf_word(nb_mf[mid * SG_BLOCK_B]), nb_id[mid * SG_BLOCK_B])) hi = mid; else lo = mid + 1;
                }
                uint32_t s = K - 1;                    // the slots from there on move down by one, the last one leaves
                for (; s > lo; --s) { nb_id[s * SG_BLOCK_B] = nb_id[(s - 1u) * SG_BLOCK_B]; nb_mf[s * SG_BLOCK_B] = nb_mf[(s - 1u) * SG_BLOCK_B]; }
                nb_id[lo * SG_BLOCK_B] = a; nb_mf[lo * SG_BLOCK_B] = (uint16_t)(m | f << 7 | (same ? 1u : 0u) << 14);
                kth_id = nb_id[(K - 1) * SG_BLOCK_B]; kth_mf = sg_mf_word(nb_mf[(K - 1) * SG_BLOCK_B]);
            }
        }
    }
    if (have) {
        uint2 *row = P.out + ((uint64_t)blockIdx.y * P.nQ + j) * K;
        for (uint32_t s = 0; s < K; ++s) row[s] = make_uint2(nb_id[s * SG_BLOCK_B], sg_mf_word(nb_mf[s * SG_BLOCK_B]));
    }
}

// ---- merge: a wavefront per query q < nQ; lane l < gy owns the sorted partial list part[(l * nQ + q) * k + 0 .. k) and keeps its head in
// registers; k times the wavefront takes the nearest head (a butterfly under fd_sig_nearer: the lists hold different candidates, so the order is
// strict until only empty slots are left) and the lane it came from steps on.  Writes out[q * k + 0 .. k).  A wavefront and not a thread per
// query: the merge runs when there are few queries and many splits, where a thread per query would leave the device idle and walk gy * k
// records one after the other.
__global__ __launch_bounds__(256) void k_sg_near_merge(const uint2 *__restrict__ part, uint32_t gy, uint32_t nQ, uint32_t k, uint2 *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t q = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= nQ) return;
    const uint2 none = make_uint2(FD_SIG_NO_ID, 0u);
    const uint2 *src = part + ((uint64_t)(lane < gy ? lane : 0u) * nQ + q) * k;
    uint32_t pos = 0;
    uint2 head = lane < gy ? src[0] : none;
    for (uint32_t r = 0; r < k; ++r) {
        uint32_t bid = head.x, bmf = head.y, bsrc = lane;
        for (int o = FD_WAVE / 2; o > 0; o >>= 1) {
            const uint32_t oid = __shfl_xor(bid, o, FD_WAVE), omf = __shfl_xor(bmf, o, FD_WAVE), osrc = __shfl_xor(bsrc, o, FD_WAVE);
            if (sg_nearer_packed(omf & 0xffu, (omf >> 8) & 0xffu, oid, bmf, bid)) { bid = oid; bmf = omf; bsrc = osrc; }
        }
        if (lane == 0) out[q * k + r] = make_uint2(bid, bmf);
        if (bsrc == lane && bid != FD_SIG_NO_ID) { ++pos; head = pos < k ? src[pos] : none; }
    }
}

#define SG_NB_MAX_SPLIT 64u      // lists a merging wavefront takes, one per lane; bounds WS_SG_NB_PART at 64 * nQ * k * 8 bytes

static int neighbors_impl(fdgpu_ctx *c, const fd_signature *Q, uint64_t nQ, const fd_signature *D, uint64_t nD, const uint32_t *exclude, uint32_t k,
                          uint32_t thr64, fd_sig_neighbor **out) {
    reset_timings(c);
    hipStream_t st = c->stream;
    const bool self = D == nullptr;
    if (self) nD = nQ;
    const uint64_t n_rec = nQ * k;
    fd_sig_neighbor *res = (fd_sig_neighbor *)fd_out_alloc(std::max<uint64_t>(n_rec, 1) * sizeof(fd_sig_neighbor));
    if (!res) FAIL(c, FDGPU_ENOMEM, "signature neighbors: out of host memory");
    const fd_sig_neighbor none = {FD_SIG_NO_ID, 0, 0, 0};
    if (!nQ || !nD) {                                   // nothing to compare: every slot is empty
        for (uint64_t i = 0; i < std::max<uint64_t>(n_rec, 1); ++i) res[i] = none;
        *out = res;
        return FDGPU_OK;
    }
    const uint32_t blocks_q = fd_grid(nQ, SG_BLOCK_B), tiles = fd_grid(nD, SG_TILE_A), most = std::min<uint32_t>(tiles, SG_NB_MAX_SPLIT);
    // as pairs_impl: enough workgroups to fill the device, no more splits than tiles; FDGPU_SG_NB_SPLIT (tests) moves the boundary
    uint32_t gy = std::max<uint32_t>(1u, std::min<uint32_t>(most, fd_grid(4096, blocks_q)));
    if (const char *e = getenv("FDGPU_SG_NB_SPLIT")) {
        const long long v = atoll(e);
        if (v > 0) gy = (uint32_t)std::min<long long>(v, most);
    }
    const size_t lds = (size_t)k * SG_NB_LDS_PER_K;
    hipError_t e = hipSuccess;
    do {
        if ((e = c->ws[WS_SG_TAB].ensure(nD * sizeof(fd_signature))) != hipSuccess) break;
        if (!self && (e = c->ws[WS_SG_TAB_B].ensure(nQ * sizeof(fd_signature))) != hipSuccess) break;
        if (exclude && (e = c->ws[WS_MISC0].ensure(nQ * 4)) != hipSuccess) break;
        if ((e = c->ws[WS_SG_NB_OUT].ensure(n_rec * sizeof(fd_sig_neighbor))) != hipSuccess) break;
        if (gy > 1 && (e = c->ws[WS_SG_NB_PART].ensure((uint64_t)gy * n_rec * sizeof(fd_sig_neighbor))) != hipSuccess) break;
        uint32_t *dD = c->ws[WS_SG_TAB].as<uint32_t>(), *dQ = self ? dD : c->ws[WS_SG_TAB_B].as<uint32_t>();
        uint32_t *dX = exclude ? c->ws[WS_MISC0].as<uint32_t>() : nullptr;
        uint2 *d_out = c->ws[WS_SG_NB_OUT].as<uint2>(), *d_part = gy > 1 ? c->ws[WS_SG_NB_PART].as<uint2>() : d_out;
        {
            StageTimer t(c, "signb_upload", (nQ + (self ? 0 : nD)) * sizeof(fd_signature) + (exclude ? nQ * 4 : 0));
            if ((e = hipMemcpyAsync(dD, self ? Q : D, nD * sizeof(fd_signature), hipMemcpyHostToDevice, st)) != hipSuccess) break;
            if (!self && (e = hipMemcpyAsync(dQ, Q, nQ * sizeof(fd_signature), hipMemcpyHostToDevice, st)) != hipSuccess) break;
            if (exclude && (e = hipMemcpyAsync(dX, exclude, nQ * 4, hipMemcpyHostToDevice, st)) != hipSuccess) break;
        }
        if ((e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sg_near), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) break;
        {
            StageTimer t(c, "signb_scan", (uint64_t)blocks_q * ((uint64_t)SG_BLOCK_B + (uint64_t)(tiles / gy + 1) * SG_TILE_A) * gy * sizeof(fd_signature));
            const sg_near_args P{dQ, dD, dX, (uint32_t)nQ, (uint32_t)nD, thr64, self ? 1u : 0u, k, d_part};
            hipLaunchKernelGGL(k_sg_near, dim3(blocks_q, gy), dim3(256), lds, st, P);
        }
        if ((e = hipGetLastError()) != hipSuccess) break;
        if (gy > 1) {
            StageTimer t(c, "signb_merge", ((uint64_t)gy + 1) * n_rec * sizeof(fd_sig_neighbor));
            hipLaunchKernelGGL(k_sg_near_merge, dim3(fd_grid(nQ, 4)), dim3(256), 0, st, d_part, gy, (uint32_t)nQ, k, d_out);
            if ((e = hipGetLastError()) != hipSuccess) break;
        }
        {
            StageTimer t(c, "signb_copy", n_rec * sizeof(fd_sig_neighbor));
            e = fd_d2h_big(c, res, d_out, n_rec * sizeof(fd_sig_neighbor));
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    } while (false);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);                 // nothing of a failed call still writes into the block
        fdgpu_free(res);
        c->err = std::string("signature neighbors: ") + hipGetErrorString(e);
        return FDGPU_EHIP;
    }
    *out = res;
    return FDGPU_OK;
}

extern "C" int fdgpu_signature_neighbors(fdgpu_ctx *c, const fd_signature *Q, uint64_t nQ, const fd_signature *D, uint64_t nD, const uint32_t *exclude, uint32_t k,
                                         uint32_t thr64, fd_sig_neighbor **out) { FD_LOCK(c);
    if (!c || !out) return FDGPU_EINVAL;
    *out = nullptr;
    if (k < 1 || k > FD_SIG_MAX_K) FAIL(c, FDGPU_EINVAL, "signature neighbors: k must be 1 .. 32");
    if (thr64 < 1 || thr64 > 64) FAIL(c, FDGPU_EINVAL, "signature neighbors: thr64 must be 1 .. 64");
    if (nQ > 0xffffffffull || (D && nD > 0xffffffffull)) FAIL(c, FDGPU_EINVAL, "signature neighbors: a table of 2^32 or more signatures");
    if (!D && exclude) FAIL(c, FDGPU_EINVAL, "signature neighbors: exclude is implied in self mode (D == NULL); pass none");
    if (nQ && !Q) FAIL(c, FDGPU_EINVAL, "signature neighbors: table Q is NULL");
    return neighbors_impl(c, Q, nQ, D, nD, exclude, k, thr64, out);
}

// ---- clusters (fdgpu_signature_clusters; the definition is include/fdgpu.h).  The table is uploaded in WALK order (the host gathers it and puts
// every record's position into its reserved word), so block w0 of the walk is W[w0 .. w0 + 256), one signature per lane as in k_sg_match.  The
// representatives chosen so far are the compact table R[0 .. *n_reps): copies of their records (the position in the reserved word), appended
// to by k_sg_cl_resolve and never uploaded again.  *n_reps lives on the device: the host sizes the grids from an upper bound (the positions
// walked so far) and never waits for it.  Per block, in stream order:
//   k_sg_cl_scan     grid (1, splits): the block against R, the tiles of R shared by blockIdx.y as in k_sg_near; every lane keeps its ONE nearest
//                    qualifying representative and writes it to part[blockIdx.y][lane].  A workgroup without a tile (blockIdx.y >= tiles of the
//                    true count) leaves at once and writes nothing.
//   k_sg_cl_resolve  one workgroup: merges the partial bests of the splits that had a tile under fd_sig_nearer, then settles the block in walk
//                    order.  The block is staged 64 signatures at a time (sg_stage_tile); tile q holds exactly the signatures of wavefront q.
//                    Wavefront q settles its own 64 in order with ballots alone: at step i lane i is a representative iff it is non-empty and
//                    has no best yet, and if so every later lane that qualifies with it and finds it nearer takes it.  It then publishes the
//                    mask of its representatives in LDS, and the wavefronts behind it compare with those.  The wavefronts before it are
//                    earlier in the walk: nothing of tile q concerns them.  So a lane's best is its nearest among R and the representatives
//                    before it in the block alike, which is the sequential walk.  A prefix sum over the workgroup gives every new representative
//                    its slot of R; the lane copies its record there, writes its result record, and thread 0 moves *n_reps.
// Nothing waits for another workgroup: no flag, no spin, no cooperative launch.  The order fd_sig_nearer is total, so neither the number of
// splits nor the width of the block changes a byte.  Records leave in walk order; the host puts them at their positions.
// With a seed table (fdgpu_signature_clusters_seeded) two launches precede the first block, once per call:
//   k_sg_cl_seed     grid (blocks, splits): every position of W against the seeds, its ONE nearest seed to part[blockIdx.y][position]
//   k_sg_cl_seed_merge  only when split: the partial bests of a position -> seed_best[position]
// and k_sg_cl_resolve starts each lane's best from seed_best.  The seeds never enter R: the walk scans what S itself adds.
#define SG_CL_MAX_SPLIT 256u     // splits of a scan: one workgroup per CU; bounds WS_SG_CL_PART at 256 * 256 * 8 bytes

struct sg_cl_args { const uint32_t *W; uint32_t *R; uint32_t *n_reps; uint2 *part; uint2 *out; uint32_t w0, nb, thr64, splits;
                    const uint2 *seed_best; };       // the seeded call: every position's nearest seed (k_sg_cl_seed), NULL without a seed table

// the lane's signature W[w0 + t] into registers (a lane beyond the block: n = 0, which is never a candidate and never a representative)
#define SG_CL_LOAD_LANE(P)                                                                                                       \
    const uint32_t t = threadIdx.x;                                                                                              \
    const bool have = t < (P).nb;                                                                                                \
    uint32_t b[64];                                                                                                              \
    uint32_t bn = 0, bpos = FD_SIG_NO_ID, bd0l = 0, bd0h = 0, bd1l = 0, bd1h = 0;                                                \
    unsigned long long b_empty = 0;                                                                                              \
    (void)bpos;                                                                                                                  \
    {                                                                                                                            \
        const uint32_t *pb = (P).W + (uint64_t)((P).w0 + (have ? t : 0u)) * FD_SIG_WORDS;                                        \
        if (have) { bn = pb[0]; bpos = pb[1]; bd0l = pb[2]; bd0h = pb[3]; bd1l = pb[4]; bd1h = pb[5]; }                          \
        _Pragma("unroll")                                                                                                        \
        for (uint32_t k = 0; k < 64; ++k) {                                                                                      \
            b[k] = have ? pb[6 + k] : FD_SIG_EMPTY;                                                                              \
            b_empty |= (unsigned long long)(b[k] == FD_SIG_EMPTY ? 1u : 0u) << k;                                                \
        }                                                                                                                        \
    }

// entry i of the staged tile, whose id is `id`, against the lane's signature: the lane's best (id, match | filled << 8 | identical << 16)
// takes it if the pair is reported and the entry is nearer.  SG_CL_TAKE: an entry of W or R, its id is its reserved word
#define SG_CL_TAKE(i) SG_CL_TAKE_ID(i, a_head[i][1])
#define SG_CL_TAKE_ID(i, id)                                                                                                     \
    {                                                                                                                            \
        uint32_t eq = 0;                                                                                                         \
        _Pragma("unroll")                                                                                                        \
        for (uint32_t k = 0; k < 64; ++k) eq += a_sk[i][k] == b[k] ? 1u : 0u;                                                    \
        const uint32_t E = (uint32_t)__popcll(a_empty[i] & b_empty);                                                             \
        const uint32_t a = (id), m = eq - E, f = 64u - E;                                                                        \
        if (fd_sig_reported(bn, a_head[i][0], eq, E, thr64) && sg_nearer_packed(m, f, a, best_mf, best_id)) {                    \
            const bool same = a_head[i][0] == bn && a_head[i][2] == bd0l && a_head[i][3] == bd0h && a_head[i][4] == bd1l && a_head[i][5] == bd1h; \
            best_id = a; best_mf = m | f << 8 | (same ? FD_SIG_IDENTICAL : 0u) << 16;                                            \
        }                                                                                                                        \
    }

// Reads W[w0 .. w0 + nb), R[0 .. *n_reps); writes part[blockIdx.y * 256 + t] for every t < 256 if it has a tile
__global__ __launch_bounds__(256) void k_sg_cl_scan(sg_cl_args P) {
    __shared__ uint32_t a_sk[SG_TILE_A][64];
    __shared__ uint32_t a_head[SG_TILE_A][6];
    __shared__ unsigned long long a_empty[SG_TILE_A];
    const uint32_t nR = *P.n_reps, tiles = (nR + SG_TILE_A - 1) / SG_TILE_A, thr64 = P.thr64;
    if (blockIdx.y >= tiles) return;                    // the grid came from an upper bound of the count
    SG_CL_LOAD_LANE(P)
    uint32_t best_id = FD_SIG_NO_ID, best_mf = 0u;
    for (uint32_t ta = blockIdx.y; ta < tiles; ta += gridDim.y) {
        sg_stage_tile(P.R, nR, (uint64_t)ta * SG_TILE_A, a_sk, a_head, a_empty);
        for (uint32_t i = 0; i < SG_TILE_A; ++i) SG_CL_TAKE(i)
    }
    P.part[blockIdx.y * SG_BLOCK_B + t] = make_uint2(best_id, best_mf);
}

// ---- the seed pass of fdgpu_signature_clusters_seeded: the seeds T[0 .. nT) never change during the walk, so every position's nearest seed is
// found once, in one launch over all blocks of the walk.  Grid (blocks of 256 positions of W, splits): a workgroup runs its 256 signatures (one
// per lane, in registers) against the tiles ta = blockIdx.y, + gridDim.y, ... of T; a seed's id is its position in T.  Every workgroup has a
// tile (the host gives no more splits than tiles).  Reads W[0 .. n), T[0 .. nT); writes part[blockIdx.y * n + w] for its positions w < n:
// seed_best itself when there is one split.
struct sg_seed_args { const uint32_t *W; const uint32_t *T; uint32_t n, nT, thr64; uint2 *part; };

__global__ __launch_bounds__(256) void k_sg_cl_seed(sg_seed_args P) {
    __shared__ uint32_t a_sk[SG_TILE_A][64];
    __shared__ uint32_t a_head[SG_TILE_A][6];
    __shared__ unsigned long long a_empty[SG_TILE_A];
    const struct { const uint32_t *W; uint32_t w0, nb; } L{P.W, blockIdx.x * SG_BLOCK_B, std::min<uint32_t>(SG_BLOCK_B, P.n - blockIdx.x * SG_BLOCK_B)};
    const uint32_t thr64 = P.thr64, tiles = (uint32_t)(((uint64_t)P.nT + SG_TILE_A - 1) / SG_TILE_A);
    SG_CL_LOAD_LANE(L)
    uint32_t best_id = FD_SIG_NO_ID, best_mf = 0u;
    for (uint32_t ta = blockIdx.y; ta < tiles; ta += gridDim.y) {
        const uint64_t a0 = (uint64_t)ta * SG_TILE_A;
        sg_stage_tile(P.T, P.nT, a0, a_sk, a_head, a_empty);
        for (uint32_t i = 0; i < SG_TILE_A; ++i) SG_CL_TAKE_ID(i, (uint32_t)a0 + i)
    }
    if (have) P.part[(uint64_t)blockIdx.y * P.n + L.w0 + t] = make_uint2(best_id, best_mf);
}

// A thread per position w < n: the nearest of part[y * n + w], y < splits, under fd_sig_nearer (the splits saw different seeds: the order is
// strict among candidates) -> seed_best[w].  The reads of a wavefront are consecutive for every y.
__global__ __launch_bounds__(256) void k_sg_cl_seed_merge(const uint2 *__restrict__ part, uint32_t splits, uint32_t n, uint2 *__restrict__ seed_best) {
    const uint64_t w = (uint64_t)blockIdx.x * SG_BLOCK_B + threadIdx.x;
    if (w >= n) return;
    uint32_t best_id = FD_SIG_NO_ID, best_mf = 0u;
#pragma unroll 4
    for (uint32_t y = 0; y < splits; ++y) {
        const uint2 c = part[(uint64_t)y * n + w];
        if (sg_nearer_packed(c.y & 0xffu, (c.y >> 8) & 0xffu, c.x, best_mf, best_id)) { best_id = c.x; best_mf = c.y; }
    }
    seed_best[w] = make_uint2(best_id, best_mf);
}

// One workgroup.  Reads part[y * 256 + t] for y < min(splits, tiles of *n_reps), W[w0 .. w0 + nb); writes out[w0 + t] for t < nb,
// R[*n_reps .. *n_reps + new representatives) (at most nb more: the host sized R for every position) and *n_reps.  With a seed table it
// also reads seed_best[w0 + t] for t < nb: the lane's best starts from its nearest seed, and the walk may still find a nearer representative
__global__ __launch_bounds__(256) void k_sg_cl_resolve(sg_cl_args P) {
    __shared__ uint32_t a_sk[SG_TILE_A][64];
    __shared__ uint32_t a_head[SG_TILE_A][6];
    __shared__ unsigned long long a_empty[SG_TILE_A];
    __shared__ unsigned long long rep_mask[SG_BLOCK_B / 64];
    __shared__ uint32_t wave_reps[SG_BLOCK_B / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, thr64 = P.thr64;
    const uint32_t nR = *P.n_reps, valid = std::min<uint32_t>(P.splits, (nR + SG_TILE_A - 1) / SG_TILE_A);
    SG_CL_LOAD_LANE(P)
    uint32_t best_id = FD_SIG_NO_ID, best_mf = 0u;
    if (P.seed_best && have) { const uint2 c = P.seed_best[P.w0 + t]; best_id = c.x; best_mf = c.y; }
    for (uint32_t y = 0; y < valid; ++y) {
        const uint2 c = P.part[y * SG_BLOCK_B + t];
        if (sg_nearer_packed(c.y & 0xffu, (c.y >> 8) & 0xffu, c.x, best_mf, best_id)) { best_id = c.x; best_mf = c.y; }
    }
    bool is_rep = false;
    for (uint32_t q = 0; q * SG_TILE_A < P.nb; ++q) {   // the same for the whole workgroup; a tile beyond the block is never staged
        sg_stage_tile(P.W, P.w0 + P.nb, (uint64_t)P.w0 + q * SG_TILE_A, a_sk, a_head, a_empty);
        if (wv == q) {
            unsigned long long mine = 0;
            for (uint32_t i = 0; i < SG_TILE_A; ++i) {
                const unsigned long long open = __ballot(bn > 0 && best_id == FD_SIG_NO_ID);      // lane i's bit is final: only lanes behind a step change
                if (!(open >> i & 1ull)) continue;      // the same for the whole wavefront
                mine |= 1ull << i;
                if (lane == i) is_rep = true;
                else if (lane > i) SG_CL_TAKE(i)
            }
            if (lane == 0) rep_mask[q] = mine;
        }
        __syncthreads();
        if (wv > q) {
            for (unsigned long long left = rep_mask[q]; left; left &= left - 1ull) {
                const uint32_t i = (uint32_t)__ffsll((long long)left) - 1u;
                SG_CL_TAKE(i)
            }
        }
    }
    // the new representatives' slots of R: ranks inside the wavefront, the wavefronts' counts through LDS
    const unsigned long long vote = __ballot(is_rep);
    if (lane == 0) wave_reps[wv] = (uint32_t)__popcll(vote);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < SG_BLOCK_B / 64; ++w) { before += w < wv ? wave_reps[w] : 0u; total += wave_reps[w]; }
    if (is_rep) {
        uint32_t *rec = P.R + (uint64_t)(nR + before + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull))) * FD_SIG_WORDS;
        rec[0] = bn; rec[1] = bpos; rec[2] = bd0l; rec[3] = bd0h; rec[4] = bd1l; rec[5] = bd1h;
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k) rec[6 + k] = b[k];
        const uint32_t filled = 64u - (uint32_t)__popcll(b_empty);
        best_id = bpos; best_mf = filled | filled << 8 | FD_SIG_IDENTICAL << 16;
    }
    if (have) P.out[P.w0 + t] = make_uint2(best_id, best_mf);
    if (threadIdx.x == 0) *P.n_reps = nR + total;
}

#define SG_CL_SEED_MAX_SPLIT 256u        // splits of the seed pass; bounds WS_SG_CL_SEED_PART at 256 * n * 8 bytes (by default: 8 MiB + 8 * n, see the header)

// the ids of a seeded call on the device are the combined ones: seed j is j, position p of S is nT + p (every record of W and so of R carries
// it in its reserved word).  The host turns them back.  T == NULL: the unseeded call, nT = 0
static int clusters_impl(fdgpu_ctx *c, const fd_signature *S, uint64_t n, const uint32_t *order, const fd_signature *T, uint64_t nT, uint32_t thr64,
                         fd_sig_neighbor **out) {
    reset_timings(c);
    hipStream_t st = c->stream;
    fd_sig_neighbor *res = (fd_sig_neighbor *)fd_out_alloc(std::max<uint64_t>(n, 1) * sizeof(fd_sig_neighbor));
    if (!res) FAIL(c, FDGPU_ENOMEM, "signature clusters: out of host memory");
    const fd_sig_neighbor none = {FD_SIG_NO_ID, 0, 0, 0};
    res[0] = none;
    if (!n) { *out = res; return FDGPU_OK; }
    // the table in walk order, every record's position in its reserved word; the records come back in walk order into `walk`
    fd_signature *W = (fd_signature *)malloc(n * sizeof(fd_signature));
    fd_sig_neighbor *walk = (fd_sig_neighbor *)malloc(n * sizeof(fd_sig_neighbor));
    if (!W || !walk) { free(W); free(walk); fdgpu_free(res); FAIL(c, FDGPU_ENOMEM, "signature clusters: out of host memory"); }
    for (uint64_t w = 0; w < n; ++w) {
        const uint64_t p = order ? order[w] : w;
        W[w] = S[p];
        W[w].reserved = (uint32_t)(nT + p);
    }
    long long forced = 0, forced_seed = 0;
    if (const char *e = getenv("FDGPU_SG_CL_SPLIT")) forced = atoll(e);
    if (const char *e = getenv("FDGPU_SG_CL_SEED_SPLIT")) forced_seed = atoll(e);
    // the seed pass: as neighbors_impl, enough workgroups to fill the device, no more splits than tiles; one when the blocks alone fill it
    const uint32_t blocks = fd_grid(n, SG_BLOCK_B), seed_most = std::min<uint32_t>(fd_grid(nT, SG_TILE_A), SG_CL_SEED_MAX_SPLIT);
    uint32_t seed_splits = nT ? std::max<uint32_t>(1u, std::min<uint32_t>(seed_most, fd_grid(4096, blocks))) : 0u;
    if (nT && forced_seed > 0) seed_splits = (uint32_t)std::min<long long>(forced_seed, seed_most);
    hipError_t e = hipSuccess;
    do {
        if ((e = c->ws[WS_SG_CL_TAB].ensure(n * sizeof(fd_signature))) != hipSuccess) break;
        if ((e = c->ws[WS_SG_CL_REPS].ensure(n * sizeof(fd_signature))) != hipSuccess) break;
        if ((e = c->ws[WS_SG_CL_OUT].ensure(n * sizeof(fd_sig_neighbor))) != hipSuccess) break;
        if ((e = c->ws[WS_SG_CL_PART].ensure((uint64_t)SG_CL_MAX_SPLIT * SG_BLOCK_B * sizeof(uint2))) != hipSuccess) break;
        if ((e = c->ws[WS_SG_CL_COUNT].ensure(64)) != hipSuccess) break;
        if (nT) {
            if ((e = c->ws[WS_SG_CL_SEEDS].ensure(nT * sizeof(fd_signature))) != hipSuccess) break;
            if ((e = c->ws[WS_SG_CL_SEED_BEST].ensure(n * sizeof(uint2))) != hipSuccess) break;
            if (seed_splits > 1 && (e = c->ws[WS_SG_CL_SEED_PART].ensure((uint64_t)seed_splits * n * sizeof(uint2))) != hipSuccess) break;
        }
        sg_cl_args P{c->ws[WS_SG_CL_TAB].as<uint32_t>(), c->ws[WS_SG_CL_REPS].as<uint32_t>(), c->ws[WS_SG_CL_COUNT].as<uint32_t>(),
                     c->ws[WS_SG_CL_PART].as<uint2>(), c->ws[WS_SG_CL_OUT].as<uint2>(), 0u, 0u, thr64, 0u, nT ? c->ws[WS_SG_CL_SEED_BEST].as<uint2>() : nullptr};
        {
            StageTimer t(c, "sigcl_upload", n * sizeof(fd_signature));
            if ((e = hipMemcpyAsync((void *)P.W, W, n * sizeof(fd_signature), hipMemcpyHostToDevice, st)) != hipSuccess) break;
            if ((e = hipMemsetAsync(P.n_reps, 0, 4, st)) != hipSuccess) break;
        }
        if (nT) {                                       // once per call, whatever n is: every block of the walk starts from seed_best
            uint32_t *dT = c->ws[WS_SG_CL_SEEDS].as<uint32_t>();
            uint2 *best = c->ws[WS_SG_CL_SEED_BEST].as<uint2>(), *part = seed_splits > 1 ? c->ws[WS_SG_CL_SEED_PART].as<uint2>() : best;
            {
                StageTimer t(c, "sigcl_seed_upload", nT * sizeof(fd_signature));
                if ((e = hipMemcpyAsync(dT, T, nT * sizeof(fd_signature), hipMemcpyHostToDevice, st)) != hipSuccess) break;
            }
            {
                StageTimer t(c, "sigcl_seed", ((uint64_t)blocks * nT + (uint64_t)seed_splits * n) * sizeof(fd_signature));
                const sg_seed_args Q{P.W, dT, (uint32_t)n, (uint32_t)nT, thr64, part};
                hipLaunchKernelGGL(k_sg_cl_seed, dim3(blocks, seed_splits), dim3(256), 0, st, Q);
            }
            if ((e = hipGetLastError()) != hipSuccess) break;
            if (seed_splits > 1) {
                StageTimer t(c, "sigcl_seed_merge", ((uint64_t)seed_splits + 1) * n * sizeof(uint2));
                hipLaunchKernelGGL(k_sg_cl_seed_merge, dim3(blocks), dim3(256), 0, st, part, seed_splits, (uint32_t)n, best);
                if ((e = hipGetLastError()) != hipSuccess) break;
            }
        }
        for (uint64_t w0 = 0; w0 < n && e == hipSuccess; w0 += SG_BLOCK_B) {
            P.w0 = (uint32_t)w0; P.nb = (uint32_t)std::min<uint64_t>(SG_BLOCK_B, n - w0);
            // at most w0 representatives so far: no more splits than their tiles; FDGPU_SG_CL_SPLIT (tests) moves the boundary
            const uint32_t most = std::min<uint32_t>(fd_grid(w0, SG_TILE_A), SG_CL_MAX_SPLIT);
            P.splits = forced > 0 ? (uint32_t)std::min<long long>(forced, most) : most;
            if (P.splits) {
                StageTimer t(c, "sigcl_scan", ((uint64_t)SG_BLOCK_B * P.splits + w0) * sizeof(fd_signature));
                hipLaunchKernelGGL(k_sg_cl_scan, dim3(1, P.splits), dim3(256), 0, st, P);
                if ((e = hipGetLastError()) != hipSuccess) break;
            }
            StageTimer t(c, "sigcl_resolve", (uint64_t)SG_BLOCK_B * (2 * sizeof(fd_signature) + P.splits * sizeof(uint2)));
            hipLaunchKernelGGL(k_sg_cl_resolve, dim3(1), dim3(256), 0, st, P);
            e = hipGetLastError();
        }
        if (e != hipSuccess) break;
        {
            StageTimer t(c, "sigcl_copy", n * sizeof(fd_sig_neighbor));
            e = fd_d2h_big(c, walk, P.out, n * sizeof(fd_sig_neighbor));
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    } while (false);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);                 // nothing of a failed call still reads the staging table
        free(W); free(walk); fdgpu_free(res);
        c->err = std::string("signature clusters: ") + hipGetErrorString(e);
        return FDGPU_EHIP;
    }
    for (uint64_t w = 0; w < n; ++w) {
        fd_sig_neighbor r = walk[w];
        if (nT && r.id != FD_SIG_NO_ID) { if (r.id < nT) r.flags |= FD_SIG_SEED; else r.id -= (uint32_t)nT; }
        res[order ? order[w] : w] = r;
    }
    free(W); free(walk);
    *out = res;
    return FDGPU_OK;
}

// what both entry points refuse before any device work, then the call
static int clusters_checked(fdgpu_ctx *c, const fd_signature *S, uint64_t n, const uint32_t *order, const fd_signature *T, uint64_t nT, uint32_t thr64,
                            fd_sig_neighbor **out) {
    if (thr64 < 1 || thr64 > 64) FAIL(c, FDGPU_EINVAL, "signature clusters: thr64 must be 1 .. 64");
    if (n > 0xffffffffull) FAIL(c, FDGPU_EINVAL, "signature clusters: a table of 2^32 or more signatures");
    if (n && !S) FAIL(c, FDGPU_EINVAL, "signature clusters: the table is NULL");
    if (nT && !T) FAIL(c, FDGPU_EINVAL, "signature clusters: the seed table is NULL");
    if (nT > 0xffffffffull || nT + n > 0xffffffffull)   // the combined ids must leave 0xFFFFFFFF free
        FAIL(c, FDGPU_EINVAL, "signature clusters: the seeds and the table together hold more than 2^32 - 1 signatures");
    if (order) {
        const uint64_t w = fd_sig_order_fault(order, n);
        if (w == FD_SIG_ORDER_NOMEM) FAIL(c, FDGPU_ENOMEM, "signature clusters: out of host memory");
        if (w != n) FAIL(c, FDGPU_EINVAL, "signature clusters: order is not a permutation of 0 .. n - 1 (entry " + std::to_string(w) + " = " + std::to_string(order[w]) + ")");
    }
    return clusters_impl(c, S, n, order, nT ? T : nullptr, nT, thr64, out);
}

extern "C" int fdgpu_signature_clusters(fdgpu_ctx *c, const fd_signature *S, uint64_t n, const uint32_t *order, uint32_t thr64, fd_sig_neighbor **out) { FD_LOCK(c);
    if (!c || !out) return FDGPU_EINVAL;
    *out = nullptr;
    return clusters_checked(c, S, n, order, nullptr, 0, thr64, out);
}

extern "C" int fdgpu_signature_clusters_seeded(fdgpu_ctx *c, const fd_signature *S, uint64_t n, const uint32_t *order, const fd_signature *T, uint64_t nT,
                                               uint32_t thr64, fd_sig_neighbor **out) { FD_LOCK(c);
    if (!c || !out) return FDGPU_EINVAL;
    *out = nullptr;
    return clusters_checked(c, S, n, order, T, nT, thr64, out);
}
