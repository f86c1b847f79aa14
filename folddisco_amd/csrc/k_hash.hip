// k_hash.hip — residue-pair enumeration + PDBTrRosetta hashing on gfx950.
//
// Replaces HOT LOOP A of the reference (src/controller/feature.rs:198-231 driven by
// src/utils/combination.rs:23-44): all ordered residue pairs (i, j), i != j, both residues
// hashable, CA-CA distance <= cutoff.
//
// Mapping: one 64-lane wavefront (= one 64-thread workgroup) per (structure, 64-residue i-tile).
// Lane l owns residue i = tile_start + l and walks j over the structure; CA_j is wave-uniform per
// step, so the CA-distance filter costs a handful of VALU issues per 64 pair tests (fd_filter_block:
// ~7 in the index build's kernels).  Only ~25 % of the tests pass, so running the ~700-instruction descriptor under
// that exec mask would idle 3/4 of the lanes; instead the passing (i, j) are compacted with
// ballot + mbcnt prefix into a per-wave LDS queue and the descriptor is evaluated in full
// 64-entry drains (one queue entry per lane).  No MFMA: this is f32/f64 VALU + irregular gather.
#include "fd_device.h"
#include "fd_geom_other.h"
// waves per SIMD the pair kernel is compiled for: 5 (88 VGPRs, 48 B of scratch) measured 15.0 ms against 16.2 (4 waves,
// 114 VGPRs) and 16.1 (6 waves, 80 VGPRs, 96 B of scratch)
#ifndef FD_EMIT_WAVES
#define FD_EMIT_WAVES 5
#endif
#define FD_MSD_BUCKETS 40u   // MSD build: bucket = top six hash bits = aa_i << 1 | aa_j >> 4 (see drain2)

// ------------------------------------------------------------------ count pass
// counts[s] += number of ordered pairs of structure s that will be emitted
__global__ __launch_bounds__(FD_WAVE) void k_pair_count(fd_batch_view B, fd_hash_consts C, uint32_t *__restrict__ counts) {
    uint32_t w = fd_xcd_remap(blockIdx.x, B.n_work);
    if (w >= B.n_work) return;
    const uint32_t s = B.wi_struct[w];
    const uint32_t r0 = B.res_off[s], r1 = B.res_off[s + 1];
    const uint32_t i = B.wi_i0[w] + threadIdx.x;
    const bool vi = i < r1 && B.hash_ok[i];
    fd_v3 cai = {0.f, 0.f, 0.f};
    if (vi) cai = fd_load3(B.ca_xyz, i);
    uint32_t cnt = 0;
    for (uint32_t j = r0; j < r1; ++j) {
        if (!B.hash_ok[j]) continue;  // wave-uniform
        fd_v3 caj = fd_load3(B.ca_xyz, j);
        float d2 = fd_dist2(cai, caj);
        cnt += (vi && i != j && !(d2 > C.d2_max)) ? 1u : 0u;
    }
    // wave reduction
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, FD_WAVE);
    if (threadIdx.x == 0 && cnt) atomicAdd(&counts[s], cnt);
}

// ------------------------------------------------------------------ emit pass
// keys/ids are written into the structure's segment [seg_off[s], seg_off[s+1]); the order inside a
// segment is unspecified (slots are claimed with one atomicAdd per 64-entry drain) — the build
// sorts by hash afterwards, and a stable sort keeps ids ascending because segments are id-major.
template <bool WRITE_IDS>
__device__ __forceinline__ void drain(const fd_batch_view &B, const fd_hash_consts &C, const uint32_t *q, uint32_t n,
                                      uint32_t i0, uint32_t r0, uint32_t s, uint32_t id, const uint64_t *seg_off,
                                      uint32_t *cursor, uint32_t *keys, uint32_t *ids) {
    const uint32_t lane = threadIdx.x;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&cursor[s], n);
    base = __shfl(base, 0, FD_WAVE);
    if (lane < n) {
        uint32_t e = q[lane];
        uint32_t i = i0 + (e >> 16), j = r0 + (e & 0xffffu);
        fd_v3 n1 = fd_load3(B.n_xyz, i), ca1 = fd_load3(B.ca_xyz, i), cb1 = fd_load3(B.cb_xyz, i);
        fd_v3 n2 = fd_load3(B.n_xyz, j), ca2 = fd_load3(B.ca_xyz, j), cb2 = fd_load3(B.cb_xyz, j);
        fd_feature f = fd_pair_feature(n1, ca1, cb1, n2, ca2, cb2);
        uint32_t h = fd_hash_enc(B.aa[i], B.aa[j], f, C.q);
        uint64_t pos = seg_off[s] + base + lane;
        keys[pos] = h;
        if (WRITE_IDS) ids[pos] = id;
    }
}

template <bool WRITE_IDS>
__global__ __launch_bounds__(FD_WAVE) void k_pair_emit(fd_batch_view B, fd_hash_consts C, const uint64_t *__restrict__ seg_off,
                                                       uint32_t *__restrict__ cursor, uint32_t *__restrict__ keys,
                                                       uint32_t *__restrict__ ids, uint32_t first_id) {
    __shared__ uint32_t q[2 * FD_WAVE];
    uint32_t w = fd_xcd_remap(blockIdx.x, B.n_work);
    if (w >= B.n_work) return;
    const uint32_t s = B.wi_struct[w];
    const uint32_t r0 = B.res_off[s], r1 = B.res_off[s + 1];
    const uint32_t i0 = B.wi_i0[w];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = i0 + lane;
    const bool vi = i < r1 && B.hash_ok[i];
    fd_v3 cai = {0.f, 0.f, 0.f};
    if (vi) cai = fd_load3(B.ca_xyz, i);
    uint32_t qn = 0;  // wave-uniform
    for (uint32_t j = r0; j < r1; ++j) {
        if (!B.hash_ok[j]) continue;
        fd_v3 caj = fd_load3(B.ca_xyz, j);
        float d2 = fd_dist2(cai, caj);
        bool pass = vi && i != j && !(d2 > C.d2_max);
        uint64_t m = __ballot(pass);
        if (m == 0) continue;
        if (pass) q[qn + fd_mbcnt(m)] = (lane << 16) | (j - r0);
        qn += (uint32_t)__popcll(m);
        if (qn >= FD_WAVE) {
            __syncthreads();
            qn -= FD_WAVE;
            drain<WRITE_IDS>(B, C, q + qn, FD_WAVE, i0, r0, s, first_id + s, seg_off, cursor, keys, ids);
            __syncthreads();
        }
    }
    if (qn) {
        __syncthreads();
        drain<WRITE_IDS>(B, C, q, qn, i0, r0, s, first_id + s, seg_off, cursor, keys, ids);
    }
}

// ------------------------------------------------------------------ frames + unordered-pair fast path
// Index-build path.  Per-residue frames (fd_make_frame) are computed once; the pair kernel visits
// every unordered pair {i < j} once and produces both ordered hashes with fd_pair_both(), which
// shares d_CA, d_CB, theta and the two pair-dependent normalised cross products between the two
// orientations (bit-exact, see fd_geom.h).  Same wave-per-(structure, i-tile) mapping and LDS
// compaction queue as above; a drain of n unordered pairs writes 2n keys.
__global__ __launch_bounds__(256) void k_frames(fd_batch_view B, uint32_t n_res, fd_frame *__restrict__ frames) {
    uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_res) return;
    fd_frame F;
    if (B.hash_ok[r]) F = fd_make_frame(fd_load3(B.n_xyz, r), fd_load3(B.ca_xyz, r), fd_load3(B.cb_xyz, r));
    else { F = fd_frame{}; F.ca = fd_load3(B.ca_xyz, r); }
    F.pad = __uint_as_float((uint32_t)B.aa[r]);   // the residue type rides in the frame's spare word (bit pattern, never computed with)
    frames[r] = F;
}

// ------------------------------------------------------------------ the distance filter of the unordered-pair kernels
// ONE place for the predicate "j > i, both hashable, !(d2 > d2_max)" of k_pair_count2, k_pair_count_msd and k_pair_emit2: what the count pass
// counts is what the emit pass emits by construction.  fd_filter_block walks one block of 64 partners j = jb .. jb + 63 for the 64-residue
// i-tile of the wavefront (lane l = residue i0 + l) and hands `step` the pass ballots of two partners at a time.  Per 64 x 2 pair tests it
// issues 8 packed f32 instructions and 2 compares, nothing else on the vector unit:
//   * CA_j is staged in LDS once per block (three planes of 64 floats) and read back with uniform-address ds_read2_b32 — no v_readlane;
//   * two partners per step in packed f32: v_pk_add_f32 (negated source), v_pk_mul_f32, v_pk_add_f32 — every half rounds like the scalar
//     instruction and the order is fd_dist2's ((dx·dx + dy·dy) + dz·dz), so each d2 has the bits fd_dist2 gives; NaN passes, as there;
//   * "i valid and hashable" is one ballot per work item (vim); "j > i" is a scalar mask: (1 << k) - 1 in the work item's first block
//     (jb == i0, the partners ARE the tile), all ones in every later one; both are ANDed to the compare's result in scalar registers;
//   * the block is cut into RUNS of partners of one kind — unhashable, or hashable of one residue type (TYPES; without it all hashable
//     partners are one kind) — by one ballot per block.  A run of unhashable partners is skipped in one scalar step, the run's type is one
//     v_readlane per run, and the loop ends at the last hashable partner (64 - clz of the hashable ballot).  In amino-acid order
//     (k_frames_perm) a block holds ~4 runs; in chain order a run may be one partner long, which is correct and only no faster.
// step(k, t, m0, m1, last): partners jb + k and jb + k + 1 of type t, m0 / m1 = the lanes whose pair passes (m1 = 0 where the run ends at
// an odd count: the second half of the packed step is computed and masked, there is no separate tail step); last = nothing follows in
// this work item (last_block's final step; it is made even where the last block has no hashable partner, with m0 = m1 = 0, so that a
// caller can flush).  run_end(t) follows the last step of every run.  s_cj: 3 * FD_WAVE + 1 floats of LDS (the odd word is read, masked,
// by a step at k = 63).  One wavefront per workgroup: LDS accesses execute in order, fd_wave_lds_fence() keeps the compiler from reordering.
typedef float fd_f2 __attribute__((ext_vector_type(2)));
#define FD_NOT_HASHABLE 0x100u

__device__ __forceinline__ bool fd_lane_of(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }   // the lane's bit of a wave-uniform mask, no VALU
// v_writelane_b32: `old` with the wave-uniform val in lane `lane` (wave-uniform, < 64).  The compiler has no builtin for it; the lane select goes
// through M0, which the compiler loads itself (the value and the lane select may not both be general scalar registers on gfx9).
__device__ __forceinline__ uint32_t fd_writelane(uint32_t old, uint32_t val, uint32_t lane) {
    asm("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(val), "{m0}"(lane));
    return old;
}

// The run structure of one block of 64 partners, from the lanes' kinds alone: what fd_filter_block walks, and what the replay of stored masks
// (fd_replay_block) walks again — both take their skips, their run ends and `last` from here.
struct fd_block_runs {
    uint64_t starts;      // bit k: a run starts at partner k
    uint32_t nkf;         // partners to walk: up to the last hashable one; an empty last block still makes the one step that carries `last`
    bool last_block;
};
__device__ __forceinline__ fd_block_runs fd_runs_of_block(uint32_t kind, uint32_t jb, uint32_t r1) {
    fd_block_runs R;
    const uint64_t okm = __ballot(kind != FD_NOT_HASHABLE);
    R.starts = __ballot(kind != (uint32_t)__shfl_up((int)kind, 1, FD_WAVE)) | 1ull;
    R.last_block = jb + FD_WAVE >= r1;
    const uint32_t nk = okm ? 64u - (uint32_t)__builtin_clzll(okm) : 0u;
    R.nkf = (R.last_block && nk == 0) ? 1u : nk;
    return R;
}
// the run that starts at partner k: its kind t, its end ke; run_last: nothing follows it in the work item
__device__ __forceinline__ void fd_run_at(const fd_block_runs &R, uint32_t kind, uint32_t k, uint32_t &t, uint32_t &ke, bool &run_last) {
    t = (uint32_t)__builtin_amdgcn_readlane((int)kind, (int)k);
    const uint64_t rest = (R.starts >> k) >> 1;
    ke = rest ? k + 1u + (uint32_t)__builtin_ctzll(rest) : (uint32_t)FD_WAVE;
    ke = ke < R.nkf ? ke : R.nkf;
    run_last = R.last_block && ke >= R.nkf;
}

template <bool TYPES, class Step, class RunEnd>
__device__ __forceinline__ void fd_filter_block(const fd_batch_view &B, float d2_max, const fd_v3 &cai, uint64_t vim, uint32_t i0, uint32_t jb, uint32_t r1,
                                                float *s_cj, Step &&step, RunEnd &&run_end) {
    const uint32_t lane = threadIdx.x;
    const uint32_t jl = jb + lane;
    fd_v3 cj = {0.f, 0.f, 0.f};
    uint32_t kind = FD_NOT_HASHABLE;
    if (jl < r1) {
        cj = fd_load3(B.ca_xyz, jl);
        if (B.hash_ok[jl]) kind = TYPES ? (uint32_t)B.aa[jl] : 0u;
    }
    fd_wave_lds_fence();
    s_cj[lane] = cj.x; s_cj[FD_WAVE + lane] = cj.y; s_cj[2 * FD_WAVE + lane] = cj.z;
    fd_wave_lds_fence();
    const fd_block_runs R = fd_runs_of_block(kind, jb, r1);
    const bool first = jb == i0;
    const fd_f2 ax = {cai.x, cai.x}, ay = {cai.y, cai.y}, az = {cai.z, cai.z};
    uint32_t k = 0;
    while (k < R.nkf) {
        uint32_t t, ke;
        bool run_last;
        fd_run_at(R, kind, k, t, ke, run_last);
        const bool dead = t == FD_NOT_HASHABLE;
        if (dead && !run_last) { k = ke; continue; }
        const uint64_t vr = dead ? 0ull : vim;
        uint64_t gt = first ? (1ull << k) - 1ull : ~0ull;      // lanes with i < jb + k
        do {
            const fd_f2 xj = {s_cj[k], s_cj[k + 1]}, yj = {s_cj[FD_WAVE + k], s_cj[FD_WAVE + k + 1]}, zj = {s_cj[2 * FD_WAVE + k], s_cj[2 * FD_WAVE + k + 1]};
            const fd_f2 dx = ax - xj, dy = ay - yj, dz = az - zj;
            const fd_f2 d2 = (dx * dx + dy * dy) + dz * dz;
            const uint64_t gt1 = gt << 1 | 1ull;
            const uint64_t m0 = __ballot(!(d2.x > d2_max)) & vr & gt;
            const uint64_t m1 = (k + 1u < ke) ? (__ballot(!(d2.y > d2_max)) & vr & gt1) : 0ull;
            gt = gt1 << 1 | 1ull;
            const uint32_t k0 = k;
            k += 2;
            step(k0, t, m0, m1, run_last && k >= ke);
        } while (k < ke);
        k = ke;
        run_end(t);
    }
}

// REPLAY of the masks the MSD count pass stored (k_pair_count_msd<true>): the same callback contract as fd_filter_block<true> — step(k, t, m0, m1,
// last), the same runs, the same `last` — without one distance: cols = the 64 words of this block in the mask table (fd_pair_mask_cols.h), word k =
// the final pass mask of partner jb + k (j > i, the tile's valid lanes and the dead runs applied; zero where the count pass made no step).  The
// partners' kinds are loaded as there, so the skips, the run ends and `last` are derived from the same ballots (fd_runs_of_block).
// A step takes its two words with ONE scalar load (s_load_dwordx4 at a wave-uniform address, straight into the scalar registers that the queue
// code wants them in): no VALU, no LDS, no CA for the filter.  The second word is read even where it is not the step's (the run ends at k + 1, or
// k = 63: the word behind the block, FD_MASK_SLACK_WORDS behind the table) and dropped.  Measured against one 8-byte vector load per lane and
// block + four v_readlane per step, and against the same scalar load requested a step ahead (HISTORY.md): this form was the fastest.
typedef uint64_t fd_u64x2 __attribute__((ext_vector_type(2), aligned(8)));
template <class Step>
__device__ __forceinline__ void fd_replay_block(const fd_batch_view &B, const uint64_t *__restrict__ cols, uint32_t jb, uint32_t r1, Step &&step) {
    const uint32_t jl = jb + threadIdx.x;
    uint32_t kind = FD_NOT_HASHABLE;
    if (jl < r1 && B.hash_ok[jl]) kind = (uint32_t)B.aa[jl];
    const fd_block_runs R = fd_runs_of_block(kind, jb, r1);
    uint32_t k = 0;
    while (k < R.nkf) {
        uint32_t t, ke;
        bool run_last;
        fd_run_at(R, kind, k, t, ke, run_last);
        if (t == FD_NOT_HASHABLE && !run_last) { k = ke; continue; }
        do {
            const fd_u64x2 m = *reinterpret_cast<const fd_u64x2 *>(cols + k);      // wave-uniform address
            const uint64_t m1 = (k + 1u < ke) ? m.y : 0ull;      // else the word belongs to the next run
            const uint32_t k0 = k;
            k += 2;
            step(k0, t, m.x, m1, run_last && k >= ke);
        } while (k < ke);
        k = ke;
    }
}

__global__ __launch_bounds__(FD_WAVE) void k_pair_count2(fd_batch_view B, fd_hash_consts C, uint32_t *__restrict__ counts) {
    __shared__ float s_cj[3 * FD_WAVE + 1];
    uint32_t w = fd_xcd_remap(blockIdx.x, B.n_work);
    if (w >= B.n_work) return;
    const uint32_t s = B.wi_struct[w];
    const uint32_t r1 = B.res_off[s + 1];
    const uint32_t i0 = B.wi_i0[w];
    const uint32_t i = i0 + threadIdx.x;
    const bool vi = i < r1 && B.hash_ok[i];
    fd_v3 cai = {0.f, 0.f, 0.f};
    if (vi) cai = fd_load3(B.ca_xyz, i);
    const uint64_t vim = __ballot(vi);
    uint32_t cnt = 0;      // unordered pairs of this lane's residue; every one is two keys
    for (uint32_t jb = i0; jb < r1; jb += FD_WAVE)
        fd_filter_block<false>(B, C.d2_max, cai, vim, i0, jb, r1, s_cj,
                               [&](uint32_t, uint32_t, uint64_t m0, uint64_t m1, bool) { cnt += (fd_lane_of(m0) ? 1u : 0u) + (fd_lane_of(m1) ? 1u : 0u); },
                               [](uint32_t) {});
    cnt *= 2u;
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, FD_WAVE);
    if (threadIdx.x == 0 && cnt) atomicAdd(&counts[s], cnt);
}

// AMINO-ACID ORDER (MSD build): one workgroup per structure sorts its residues by type — a stable counting sort, hashable residues first,
// unhashable and out-of-range types last — and writes permuted copies of what the pair kernels read per residue (CA, hashable flag, type)
// plus src_perm[p], the residue that lands at p: the count pass builds the frames through it (k_pair_count_msd).  A 64-residue tile then
// holds ~4 residue types instead of ~15, which is what keeps the bucket runs of a drain long (k_pair_emit2<.., MSD>).  Inside a type the
// residues keep residue order: a trip of 256 residues is ranked by one ballot per type and wavefront and the wavefronts' counts, not by
// LDS atomics on the slot counters, so the order — and with it the emitted stream — is the same in every run.
__global__ __launch_bounds__(256) void k_frames_perm(fd_batch_view B, float *__restrict__ ca_perm, uint8_t *__restrict__ ok_perm, uint8_t *__restrict__ aa_perm,
                                                     uint32_t *__restrict__ src_perm, unsigned long long *__restrict__ wide_flag) {
    __shared__ uint32_t cnt[32], cur[32], wcnt[4][32];
    const uint32_t s = blockIdx.x, lane = threadIdx.x & (FD_WAVE - 1u), wave = threadIdx.x / FD_WAVE;
    const uint32_t r0 = B.res_off[s], r1 = B.res_off[s + 1];
    if (threadIdx.x < 32) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t r = r0 + threadIdx.x; r < r1; r += 256) {      // the totals per type: their order does not matter
        const uint32_t a = B.aa[r];
        atomicAdd(&cnt[(B.hash_ok[r] && a < 20u) ? a : 20u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t run = 0; for (int k = 0; k < 21; ++k) { cur[k] = run; run += cnt[k]; } }
    __syncthreads();
    for (uint32_t rb = r0; rb < r1; rb += 256) {      // workgroup-uniform trips: the barriers inside are reached by every thread
        const uint32_t r = rb + threadIdx.x;
        uint32_t a = 0, cls = 21u;      // 21: no residue
        bool ok = false;
        if (r < r1) {
            a = B.aa[r];
            ok = B.hash_ok[r] != 0;
            if (ok && a >= 20u) {      // a residue type outside map_aa_to_u8's 0..19 marked hashable: forty buckets cannot hold it — the build is redone with the
                ok = false;            // structure-major 8-byte path, which hashes whatever the caller passed (wide_flag)
                if (wide_flag) atomicOr(wide_flag, 1ull);
            }
            cls = ok ? a : 20u;
        }
        uint64_t mine = 0;      // the lanes of this wavefront with this lane's type
        uint32_t wc = 0;        // lane k: residues of type k in this wavefront
#pragma unroll 1      // unrolled, the 21 masks are all held in scalar registers at once and some are spilled
        for (uint32_t k = 0; k < 21u; ++k) {
            const uint64_t m = __ballot(cls == k);
            if (cls == k) mine = m;
            if (lane == k) wc = (uint32_t)__popcll(m);
        }
        if (lane < 21u) wcnt[wave][lane] = wc;
        __syncthreads();
        if (r < r1) {
            uint32_t p = r0 + cur[cls] + fd_mbcnt(mine);      // the type's first free slot + the residues of the type in front of this one
            for (uint32_t v = 0; v < wave; ++v) p += wcnt[v][cls];
            const fd_v3 ca = fd_load3(B.ca_xyz, r);
            ca_perm[3ull * p] = ca.x; ca_perm[3ull * p + 1] = ca.y; ca_perm[3ull * p + 2] = ca.z;
            ok_perm[p] = ok ? 1 : 0;
            aa_perm[p] = (uint8_t)a;
            src_perm[p] = r;
        }
        __syncthreads();
        if (threadIdx.x < 21u) cur[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
        __syncthreads();
    }
}

// count pass of the MSD build: counts[bucket * n_work + w] = keys of work item w that fall into the bucket (both orientations of every
// unordered pair: (aa_i, aa_j >> 4) and (aa_j, aa_i >> 4)).  Every work item writes all forty of its entries with plain stores, zeros
// included, so the table needs no clearing and nothing of an earlier call shows; its exclusive scan gives every work item private,
// contiguous slots in every bucket (work items are in structure order: the stream stays structure-major inside a bucket).  The partners
// come in runs of one residue type (fd_filter_block; amino-acid order makes them ~16 long), so ONE per-lane pass counter per run serves
// both orientations: at the end of the run it goes to the lane's forward counter of the run's half (c_lo / c_hi) and, as the reverse keys
// of bucket (aa_j, aa_i >> 4), into the forty LDS counters.  B = the permuted view.
// A work item is exactly one 64-residue tile of the permuted order, so every frame belongs to one work item: in front of the filter loop
// lane l gathers N and CB of the residue that landed at i0 + l (src_perm; n_xyz / cb_xyz are the batch's arrays in chain order), builds
// the frame and stores it for the emit pass.  The kernel is bound by the filter loop's scalar instructions; the frames ride in its idle
// vector and memory slots.
// STORE: the pass masks of every step are kept for the emit pass (fd_replay_block), which then runs no distance test.  m0 / m1 are final words in
// scalar registers; a step puts them into lanes k and k + 1 of one register pair (four v_writelane) and the block's 64 words leave with one
// coalesced 8-byte vector store per lane.  The pair starts every block at zero and every lane stores, so the dead runs, the odd run tails, the partners behind the
// last hashable one and the padding columns are zero words written by THIS call: nothing of an earlier call shows and nothing is cleared.  The
// counts are taken from the very words that are stored.
template <bool STORE>
__global__ __launch_bounds__(FD_WAVE) void k_pair_count_msd(fd_batch_view B, fd_hash_consts C, const float *__restrict__ n_xyz, const float *__restrict__ cb_xyz,
                                                            const uint32_t *__restrict__ src_perm, fd_frame *__restrict__ frames, uint32_t *__restrict__ counts,
                                                            uint64_t *__restrict__ masks) {
    __shared__ uint32_t s_cnt[FD_WAVE];
    __shared__ float s_cj[3 * FD_WAVE + 1];
    uint32_t w = fd_xcd_remap(blockIdx.x, B.n_work);
    if (w >= B.n_work) return;
    const uint32_t s = B.wi_struct[w];
    const uint32_t r1 = B.res_off[s + 1];
    const uint32_t i0 = B.wi_i0[w];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = i0 + lane;
    const bool vi = i < r1 && B.hash_ok[i];
    fd_v3 cai = {0.f, 0.f, 0.f};
    uint32_t aai = 0;
    if (vi) { cai = fd_load3(B.ca_xyz, i); aai = B.aa[i]; }
    if (i < r1) {
        fd_frame F;
        if (vi) { const uint32_t src = src_perm[i]; F = fd_make_frame(fd_load3(n_xyz, src), cai, fd_load3(cb_xyz, src)); }
        else { F = fd_frame{}; F.ca = fd_load3(B.ca_xyz, i); }
        F.pad = __uint_as_float((uint32_t)B.aa[i]);      // the residue type rides in the frame's spare word (bit pattern, never computed with)
        frames[i] = F;
    }
    s_cnt[lane] = 0;
    __syncthreads();
    const uint64_t vim = __ballot(vi);
    uint32_t c_lo = 0, c_hi = 0, run = 0;
    const uint32_t hi_i = aai >> 4;
    uint2 *mrow = STORE ? reinterpret_cast<uint2 *>(masks + B.wi_col[w]) + lane : nullptr;      // this lane's word of the work item's first block
    for (uint32_t jb = i0; jb < r1; jb += FD_WAVE) {
        uint32_t c_x = 0, c_y = 0;      // lane k: the mask of partner jb + k
        fd_filter_block<true>(B, C.d2_max, cai, vim, i0, jb, r1, s_cj,
                              [&](uint32_t k, uint32_t, uint64_t m0, uint64_t m1, bool) {
                                  run += (fd_lane_of(m0) ? 1u : 0u) + (fd_lane_of(m1) ? 1u : 0u);
                                  if (STORE) {
                                      // m1 first, at lane min(k + 1, 63): a step at k = 63 has m1 = 0 and no lane 64 — its zero goes where m0 follows
                                      const uint32_t k1 = k + 1u < FD_WAVE ? k + 1u : FD_WAVE - 1u;
                                      c_x = fd_writelane(c_x, (uint32_t)m1, k1);
                                      c_y = fd_writelane(c_y, (uint32_t)(m1 >> 32), k1);
                                      c_x = fd_writelane(c_x, (uint32_t)m0, k);
                                      c_y = fd_writelane(c_y, (uint32_t)(m0 >> 32), k);
                                  }
                              },
                              [&](uint32_t t) {      // t: wave-uniform; FD_NOT_HASHABLE only with run == 0 in every lane
                                  if (t >= 16u) c_hi += run; else c_lo += run;
                                  if (run) atomicAdd(&s_cnt[(t * 2u + hi_i) & (FD_WAVE - 1u)], run);
                                  run = 0;
                              });
        if (STORE) { *mrow = make_uint2(c_x, c_y); mrow += FD_WAVE; }
    }
    if (c_lo) atomicAdd(&s_cnt[aai * 2u], c_lo);
    if (c_hi) atomicAdd(&s_cnt[aai * 2u + 1u], c_hi);
    __syncthreads();
    if (lane < FD_MSD_BUCKETS) counts[(uint64_t)lane * B.n_work + w] = s_cnt[lane];
}

__device__ __forceinline__ fd_frame load_frame(const fd_frame *__restrict__ frames, uint32_t r) {
    const float4 *p = reinterpret_cast<const float4 *>(frames + r);
    float4 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4];
    fd_frame F;
    F.ca = {a.x, a.y, a.z}; F.cb = {a.w, b.x, b.y}; F.r1 = {b.z, b.w, c.x}; F.t1 = {c.y, c.z, c.w};
    F.len = d.x; F.pad = d.y; F.s2 = {d.z, d.w, e.x}; F.nv2 = {e.y, e.z, e.w};
    return F;
}
// the hot part of a frame (fd_geom.h) from its four 16-byte words; s2 / nv2 stay zero: fd_pair_both_spec reads neither
__device__ __forceinline__ fd_frame hot_frame(const float4 &a, const float4 &b, const float4 &c, const float4 &d) {
    fd_frame F{};
    F.ca = {a.x, a.y, a.z}; F.cb = {a.w, b.x, b.y}; F.r1 = {b.z, b.w, c.x}; F.t1 = {c.y, c.z, c.w};
    F.len = d.x; F.pad = d.y;
    return F;
}

// IDS16: 6-byte elements — key = hash << 2 | (s >> 16), 16-bit payload = s & 0xffff (s = structure index inside the shard)
// exact table evaluation, out of line: the fallback of the speculative path (and the whole path with FDGPU_EXACT=1)
__device__ __attribute__((noinline)) uint2 pair_both_tab_exact(const fd_frame *__restrict__ frames, uint32_t i, uint32_t j, uint32_t aai,
                                                               uint32_t aaj, float dist_disc, float ang_disc, const uint32_t *tab) {
    fd_frame Fi = load_frame(frames, i), Fj = load_frame(frames, j);
    fd_quant q;
    q.dist_disc = dist_disc; q.ang_disc = ang_disc; q.ang2_disc = 0.0f; q.type = FD_HASH_PDBTR;
    uint32_t a, b;
    fd_pair_both_tab(Fi, Fj, aai, aaj, q, tab, &a, &b);
    return make_uint2(a, b);
}

// MSD (index build, 6-byte elements, default encoding): the keys leave the kernel already partitioned by the top six hash bits — bucket =
// hash >> 24 = aa_i << 1 | aa_j >> 4, forty of them — into a BUCKET-major stream (inside a bucket structure-major, so the stable sort that
// follows still leaves ids ascending inside every hash).  seg_off is then a [bucket][work item] table (k_pair_count_msd): a work item owns
// private, contiguous slots in every bucket, and their forty starts are its running cursor in LDS (s_boff).  A drain counts its keys per
// bucket in LDS (two ds_add_rtn per lane), stores every key at cursor + its rank inside the drain and advances the cursor by the counts:
// no global atomic, no memory shared with another workgroup.  The residues of a structure are visited in amino-acid order
// (k_frames_perm), so a drain touches a handful of buckets and the partial lines of one bucket's run are completed in L2 by the drains
// that follow.  The sort then needs three 8-bit passes, not four.
template <int TAB, bool IDS16, bool MSD, bool DT = false>
__device__ __forceinline__ void drain2(const fd_batch_view &B, const fd_frame *__restrict__ frames, const fd_hash_consts &C,
                                       const uint32_t *tab, const uint32_t *q, uint32_t n, uint32_t i0, uint32_t r0, uint32_t s, uint32_t id,
                                       const uint64_t *seg_off, uint32_t *cursor, uint32_t *keys, void *ids, const float4 *s_fi,
                                       uint32_t *s_bc, uint64_t *s_boff) {
    const uint32_t lane = threadIdx.x;
    uint32_t base = 0, slots = 0;
    if (!MSD) {
        if (lane == 0) base = atomicAdd(&cursor[s], 2u * n);
        base = __shfl(base, 0, FD_WAVE);
    } else {
        // the buckets of a drain's keys are known before any geometry (the queue entry carries the partner's residue type): count per
        // bucket in LDS; a lane's two results are its keys' ranks inside the drain
        s_bc[lane] = 0;
        fd_wave_lds_fence();
        if (lane < n) {
            const uint32_t e = q[lane], il = (e >> 16) & 63u, aj = e >> 22;
            const uint32_t ai = TAB == 2 ? __float_as_uint(s_fi[192 + il].y) : (uint32_t)B.aa[i0 + il];
            const uint32_t bf = ai * 2u + (aj >> 4), br = aj * 2u + (ai >> 4);
            slots = atomicAdd(&s_bc[bf], 1u) | atomicAdd(&s_bc[br], 1u) << 8 | bf << 16 | br << 24;      // one register across the descriptor
        }
    }
    uint32_t h_ij = 0, h_ji = 0, aai = 0, aaj = 0;
    if (lane < n) {
        uint32_t e = q[lane];
        uint32_t i = i0 + ((e >> 16) & 63u), j = r0 + (e & 0xffffu);
        if (TAB == 2) {
            // hot frame of i from the work item's LDS-staged residue tile ([k][lane] float4 planes), hot frame of j from L2
            const uint32_t il = (e >> 16) & 63u;
            const fd_frame Fi = hot_frame(s_fi[il], s_fi[64 + il], s_fi[128 + il], s_fi[192 + il]);
            const float4 *pj = reinterpret_cast<const float4 *>(frames + j);
            const fd_frame Fj = hot_frame(pj[0], pj[1], pj[2], pj[3]);
            aai = __float_as_uint(Fi.pad); aaj = __float_as_uint(Fj.pad);
#if defined(FD_EMIT_STUB) && FD_EMIT_STUB == 1
            // measurement build (tools/attrib_emit.sh): the drain without the descriptor — frames loaded, slots claimed, keys stored
            h_ij = aai << 25 | aaj << 20 | (__float_as_uint(Fj.ca.x) & 0xfffffu); h_ji = aaj << 25 | aai << 20 | (__float_as_uint(Fi.ca.x) & 0xfffffu);
            if (false)
#endif
            if (!fd_pair_both_spec<DT>(Fi, Fj, aai, aaj, C.q, tab, tab + 32, &h_ij, &h_ji, tab + 64)) {
                uint2 h = pair_both_tab_exact(frames, i, j, B.aa[i], B.aa[j], C.q.dist_disc, C.q.ang_disc, tab);
                h_ij = h.x; h_ji = h.y;
                if (C.spec_miss) atomicAdd(C.spec_miss, 1ull);
            }
        } else if (TAB == 1) {
            uint2 h = pair_both_tab_exact(frames, i, j, B.aa[i], B.aa[j], C.q.dist_disc, C.q.ang_disc, tab);
            h_ij = h.x; h_ji = h.y;
        } else {
            fd_frame Fi = load_frame(frames, i), Fj = load_frame(frames, j);
            fd_pair_both(Fi, Fj, B.aa[i], B.aa[j], C.q, &h_ij, &h_ji);
        }
    }
    if (MSD) {
        if (lane < n) {
            const uint32_t sf = slots & 255u, sr = (slots >> 8) & 255u, bf = (slots >> 16) & 255u, br = slots >> 24;
            // the bucket comes from the residue types like in the count pass (== hash >> 24 unless a saturated distance field bled into
            // the type bits: such a hash raises wide_flag and the build is redone with 8-byte elements; its key still lands in a counted slot)
            if ((((h_ij | h_ji) >> 30) || (h_ij >> 24) != bf || (h_ji >> 24) != br) && C.wide_flag) atomicOr(C.wide_flag, 1ull);
            const uint64_t pf = s_boff[bf] + sf, pr = s_boff[br] + sr;      // 64 bits: a build call may hold more than 2^32 keys
            // the position says which bucket (the top six hash bits); the other 24 are the three sorted digits: the u32 plane keeps
            // hash[7:0] << 24 | s (s < 2^24), the u16 plane hash[23:8] — a histogram pass of the sort reads only its digit's plane
            keys[pf] = (h_ij << 24) | s;
            keys[pr] = (h_ji << 24) | s;
            ((uint16_t *)ids)[pf] = (uint16_t)(h_ij >> 8);
            ((uint16_t *)ids)[pr] = (uint16_t)(h_ji >> 8);
        }
        fd_wave_lds_fence();
        if (lane < FD_MSD_BUCKETS) s_boff[lane] += s_bc[lane];      // the next drain's first slot in every bucket
        return;
    }
    if (lane < n) {
        // --multiple-bins: the structure's segment holds seg_mul copies of its pair list (one per bin pair), so the stream stays
        // structure-major and the stable sort by hash keeps ids ascending inside every posting list
        const uint64_t so = seg_off[s];
        uint64_t pos = so * C.seg_mul + (uint64_t)C.seg_cfg * (seg_off[s + 1] - so) + base + lane;
        if (IDS16) {
            if (((h_ij | h_ji) >> 30) && C.wide_flag) atomicOr(C.wide_flag, 1ull);   // does not fit hash << 2: the caller rebuilds with 8-byte elements
            uint32_t hi = s >> 16;
            uint16_t lo = (uint16_t)(s & 0xffffu);
            keys[pos] = (h_ij << 2) | hi;
            keys[pos + n] = (h_ji << 2) | hi;
            ((uint16_t *)ids)[pos] = lo;
            ((uint16_t *)ids)[pos + n] = lo;
        } else {
            keys[pos] = h_ij;
            keys[pos + n] = h_ji;
            ((uint32_t *)ids)[pos] = id;
            ((uint32_t *)ids)[pos + n] = id;
        }
    }
}

// MASKS (MSD only): the pass masks come from the table the count pass stored (fd_replay_block) instead of from fd_filter_block — the kernel
// then holds no CA of its own tile, no staged partner CAs (s_cj) and makes no distance test; the queue, the drain site and drain2 are the same.
template <int TAB, bool IDS16, bool MSD, bool DT = false, bool MASKS = false>
__global__ __launch_bounds__(FD_WAVE, FD_EMIT_WAVES) void k_pair_emit2(fd_batch_view B, const fd_frame *__restrict__ frames, fd_hash_consts C,
                                                        const uint64_t *__restrict__ seg_off, uint32_t *__restrict__ cursor,
                                                        uint32_t *__restrict__ keys, void *__restrict__ ids, uint32_t first_id,
                                                        const uint64_t *__restrict__ masks) {
    static_assert(!MASKS || MSD, "the mask table belongs to the MSD build");
    __shared__ uint32_t q[3 * FD_WAVE];      // a step queues up to 2 x 64 entries on top of the < 64 left by the drains before it
    __shared__ float s_cj[MASKS ? 1 : 3 * FD_WAVE + 1];
    __shared__ uint32_t tab[DT ? 64 + FD_DIST_NTHR + 1 : 64];   // [0,27) exact table (bit patterns), [32,59) the same with float thresholds for the speculative path,
                                                                 // DT: [64, 64 + FD_DIST_NTHR) the squared-distance breakpoints of the two distance fields
    uint32_t w = fd_xcd_remap(blockIdx.x, B.n_work);
    if (w >= B.n_work) return;
    if (TAB) {
        if (DT && threadIdx.x < FD_DIST_NTHR) tab[64 + threadIdx.x] = fd_dist_thr_bits[threadIdx.x];
        if (threadIdx.x == 0) {
            fd_fill_bintab(tab);
            for (int k = 0; k < FD_BINTAB_WORDS; ++k) tab[32 + k] = tab[k];
            for (int m = 0; m < 4; ++m)
                for (int k = 0; k < 4; ++k) { uint32_t v = tab[32 + 7 + 5 * m + k]; tab[32 + 7 + 5 * m + k] = v > 0x7f7fffffu ? 0x7f7fffffu : v; }
        }
        __syncthreads();
    }
    const uint32_t s = B.wi_struct[w];
    const uint32_t r0 = B.res_off[s], r1 = B.res_off[s + 1];
    const uint32_t i0 = B.wi_i0[w];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = i0 + lane;
    // LDS staging of the work item's residue tile: the hot 64 bytes of the 64 frames of the i side (4 KB), plane-major so that the fill
    // is conflict-free; every drain reads its i frames from here instead of gathering them from L2 again
    __shared__ float4 s_fi[4 * FD_WAVE];
    if (TAB == 2 && i < r1) {
        const float4 *fp = reinterpret_cast<const float4 *>(frames + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) s_fi[k * FD_WAVE + lane] = fp[k];
    }
    __shared__ uint32_t s_bc[MSD ? FD_WAVE : 1];
    __shared__ uint64_t s_boff[MSD ? FD_MSD_BUCKETS : 1];      // forty, not 64: the workgroup stays below 8 KB, 20 of them on a CU
    if (MSD && lane < FD_MSD_BUCKETS) s_boff[lane] = seg_off[(uint64_t)lane * B.n_work + w];      // where the work item's keys of every bucket start: its cursor
    __syncthreads();
    const uint32_t lane16 = lane << 16;
    uint32_t qn = 0;  // wave-uniform
    uint32_t jrel = i0 - r0;      // the block's first partner, relative to the structure
    // single drain site (two inlined copies of the descriptor code would not fit the I-cache): the two ballots of a step are queued one
    // after the other in front of it, and the step that the filter (or the replay) marks `last` flushes what is left (up to three drains).
    auto step = [&](uint32_t k, uint32_t t, uint64_t m0, uint64_t m1, bool last) {
        // queue entry: lane << 16 | partner (relative to the structure); MSD: bits 22-26 = the partner's residue type, the run's
        const uint32_t tag = (MSD ? t << 22 : 0u) | (jrel + k);
        if (m0) {
            if (fd_lane_of(m0)) q[__builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m0, qn))] = lane16 | tag;
            qn += (uint32_t)__popcll(m0);
        }
        if (m1) {
            if (fd_lane_of(m1)) q[__builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, qn))] = lane16 | (tag + 1u);
            qn += (uint32_t)__popcll(m1);
        }
        while (qn >= FD_WAVE || (last && qn)) {
            fd_wave_lds_fence();
            uint32_t n = qn < FD_WAVE ? qn : FD_WAVE;
            qn -= n;
            drain2<TAB, IDS16, MSD, DT>(B, frames, C, tab, q + qn, n, i0, r0, s, first_id + s, seg_off, cursor, keys, ids, s_fi, s_bc, s_boff);
            fd_wave_lds_fence();
        }
    };
    if constexpr (MASKS) {
        const uint64_t *cols = masks + B.wi_col[w];      // the work item's columns: whole blocks of 64 (fd_pair_mask_cols.h)
        for (uint32_t jb = i0; jb < r1; jb += FD_WAVE, jrel += FD_WAVE, cols += FD_WAVE) fd_replay_block(B, cols, jb, r1, step);
    } else {
        const bool vi = i < r1 && B.hash_ok[i];
        fd_v3 cai = {0.f, 0.f, 0.f};
        if (vi) cai = fd_load3(B.ca_xyz, i);
        const uint64_t vim = __ballot(vi);
        for (uint32_t jb = i0; jb < r1; jb += FD_WAVE, jrel += FD_WAVE) fd_filter_block<MSD>(B, C.d2_max, cai, vim, i0, jb, r1, s_cj, step, [](uint32_t) {});
    }
}

// ------------------------------------------------------------------ ordered variant (API S1, sort_dedup = 0)
// Same pairs, but written in the reference's row-major (i, j) order: one lane per i computes its
// row offset by a prefix over row counts.  Used for parity tests of the raw hash list; not on the
// index-build fast path.
__global__ __launch_bounds__(FD_WAVE) void k_row_count(fd_batch_view B, fd_hash_consts C, uint32_t *__restrict__ row_cnt, float cutoff) {
    uint32_t w = fd_xcd_remap(blockIdx.x, B.n_work);
    if (w >= B.n_work) return;
    const uint32_t s = B.wi_struct[w];
    const uint32_t r0 = B.res_off[s], r1 = B.res_off[s + 1];
    const uint32_t i = B.wi_i0[w] + threadIdx.x;
    if (i >= r1) return;
    if (fd_own_descriptor(C.q.type)) {   // the encodings with their own descriptor and acceptance rule (fd_geom_other.h)
        uint32_t cnt = 0;
        if (B.aa[i] != 255)
            for (uint32_t j = r0; j < r1; ++j)
                cnt += (j != i && B.aa[j] != 255 && fd_accept_other(C.q.type, B, r0, r1, i, j, cutoff)) ? 1u : 0u;
        row_cnt[i] = cnt;
        return;
    }
    const bool vi = B.hash_ok[i];
    fd_v3 cai = fd_load3(B.ca_xyz, i);
    uint32_t cnt = 0;
    for (uint32_t j = r0; j < r1; ++j) {
        if (!B.hash_ok[j]) continue;
        float d2 = fd_dist2(cai, fd_load3(B.ca_xyz, j));
        cnt += (vi && i != j && !(d2 > C.d2_max)) ? 1u : 0u;
    }
    row_cnt[i] = cnt;
}

// ids (optional): the structure id first_id + s of every entry, or with ids_partner its partner residue j (batch residue index) — the
// row start row_off[i] gives i, so (hash, i, j) is what collect_hash_id_pos walks (controller/summary.rs:632-690)
__global__ __launch_bounds__(FD_WAVE) void k_row_emit(fd_batch_view B, fd_hash_consts C, const uint64_t *__restrict__ row_off,
                                                      uint32_t *__restrict__ keys, float cutoff, uint32_t *__restrict__ ids, uint32_t first_id, int ids_partner) {
    uint32_t w = fd_xcd_remap(blockIdx.x, B.n_work);
    if (w >= B.n_work) return;
    const uint32_t s = B.wi_struct[w];
    const uint32_t r0 = B.res_off[s], r1 = B.res_off[s + 1];
    const uint32_t i = B.wi_i0[w] + threadIdx.x;
    if (i >= r1) return;
    if (fd_own_descriptor(C.q.type)) {
        if (B.aa[i] == 255) return;
        uint64_t pos = row_off[i];
        float f[FD_NFEAT];
        for (uint32_t j = r0; j < r1; ++j) {
            if (j == i || B.aa[j] == 255 || !fd_feature_other(C.q.type, B, r0, r1, i, j, cutoff, f)) continue;
            if (ids) ids[pos] = ids_partner ? j : first_id + s;
            keys[pos++] = fd_hash_other(C.q.type, f, C.q);
        }
        return;
    }
    if (!B.hash_ok[i]) return;
    fd_v3 n1 = fd_load3(B.n_xyz, i), ca1 = fd_load3(B.ca_xyz, i), cb1 = fd_load3(B.cb_xyz, i);
    uint32_t aa1 = B.aa[i];
    uint64_t pos = row_off[i];
    for (uint32_t j = r0; j < r1; ++j) {
        if (!B.hash_ok[j] || i == j) continue;
        fd_v3 ca2 = fd_load3(B.ca_xyz, j);
        if (fd_dist2(ca1, ca2) > C.d2_max) continue;
        fd_v3 n2 = fd_load3(B.n_xyz, j), cb2 = fd_load3(B.cb_xyz, j);
        fd_feature f = fd_pair_feature(n1, ca1, cb1, n2, ca2, cb2);
        if (ids) ids[pos] = ids_partner ? j : first_id + s;
        keys[pos++] = fd_hash_enc(aa1, B.aa[j], f, C.q);
    }
}

// aa / cb_valid -> hash_ok
__global__ void k_hash_ok(const uint8_t *__restrict__ aa, const uint8_t *__restrict__ cb_valid, uint8_t *__restrict__ ok, uint64_t n) {
    uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) ok[k] = (aa[k] != 255 && (cb_valid == nullptr || cb_valid[k])) ? 1 : 0;
}

// ------------------------------------------------------------------ start-up known-answer test (fdgpu_create)
// The catalytic triad of query/4CHA.pdb (HIS B57, ASP B102, SER C195) and its six PDBTrRosetta hashes, the literals of the
// reference's own test (controller/graph.rs:71-79).  Every ordered pair is evaluated three ways — the generic chain
// (fd_pair_feature + fd_hash_pdbtr: restated sinf/cosf/acosf/atan2f), the exhaustive-table form (fd_pair_both_tab) and the
// speculative form (fd_pair_both_spec, exact fallback on refusal) — so a build whose arithmetic drifts (fast-math, FMA contraction,
// a different table generation) fails loudly instead of producing a subtly different index.
__global__ void k_selfcheck(fd_quant q, uint32_t *__restrict__ out /*[24]*/) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const fd_v3 N[3] = {{6.661f, 8.291f, 43.860f}, {10.483f, 7.756f, 49.260f}, {5.260f, -1.068f, 41.296f}};
    const fd_v3 CA[3] = {{6.994f, 8.354f, 42.405f}, {9.429f, 7.479f, 48.266f}, {5.547f, 0.158f, 42.050f}};
    const fd_v3 CB[3] = {{8.251f, 7.488f, 42.026f}, {10.033f, 6.489f, 47.255f}, {5.773f, 1.360f, 41.130f}};
    const uint32_t AA[3] = {8u, 3u, 15u};
    const int PI[6] = {1, 1, 0, 0, 2, 2}, PJ[6] = {0, 2, 1, 2, 1, 0};   // B102->B57, B102->C195, B57->B102, B57->C195, C195->B102, C195->B57
    uint32_t tab[64 + FD_DIST_NTHR + 1];
    fd_fill_bintab(tab);
    for (int k = 0; k < FD_BINTAB_WORDS; ++k) tab[32 + k] = tab[k];
    for (int m = 0; m < 4; ++m)
        for (int k = 0; k < 4; ++k) { uint32_t v = tab[32 + 7 + 5 * m + k]; tab[32 + 7 + 5 * m + k] = v > 0x7f7fffffu ? 0x7f7fffffu : v; }
    for (int k = 0; k < FD_DIST_NTHR; ++k) tab[64 + k] = fd_dist_thr_bits[k];
    fd_frame F[3];
    for (int r = 0; r < 3; ++r) F[r] = fd_make_frame(N[r], CA[r], CB[r]);
    for (int k = 0; k < 6; ++k) {
        const int i = PI[k], j = PJ[k];
        out[k] = fd_hash_pdbtr(AA[i], AA[j], fd_pair_feature(N[i], CA[i], CB[i], N[j], CA[j], CB[j]), q);
        uint32_t a, b;
        fd_pair_both_tab(F[i], F[j], AA[i], AA[j], q, tab, &a, &b);
        out[6 + k] = a;
        if (!fd_pair_both_spec(F[i], F[j], AA[i], AA[j], q, tab, tab + 32, &a, &b)) fd_pair_both_tab(F[i], F[j], AA[i], AA[j], q, tab, &a, &b);
        out[12 + k] = a;
        // ... and with the distance fields from the squared-distance table (the index build's form; valid for the default 16 distance bins the check runs with)
        if (!fd_pair_both_spec<true>(F[i], F[j], AA[i], AA[j], q, tab, tab + 32, &a, &b, tab + 64)) fd_pair_both_tab(F[i], F[j], AA[i], AA[j], q, tab, &a, &b);
        out[18 + k] = a;
    }
}

// ------------------------------------------------------------------ launchers (called from fd_api_build.hip)
extern "C++" {
void fd_launch_selfcheck(const fd_quant &q, uint32_t *out, hipStream_t st) { hipLaunchKernelGGL(k_selfcheck, dim3(1), dim3(64), 0, st, q, out); }
void fd_launch_hash_ok(const uint8_t *aa, const uint8_t *cb_valid, uint8_t *ok, uint64_t n, hipStream_t st) {
    if (!n) return;
    hipLaunchKernelGGL(k_hash_ok, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, aa, cb_valid, ok, n);
}
static inline unsigned grid_for(uint32_t n_work) { return ((n_work + 7u) / 8u) * 8u; }
void fd_launch_pair_count(const fd_batch_view &B, const fd_hash_consts &C, uint32_t *counts, hipStream_t st) {
    if (!B.n_work) return;
    hipLaunchKernelGGL(k_pair_count, dim3(grid_for(B.n_work)), dim3(FD_WAVE), 0, st, B, C, counts);
}
void fd_launch_pair_emit(const fd_batch_view &B, const fd_hash_consts &C, const uint64_t *seg_off, uint32_t *cursor,
                         uint32_t *keys, uint32_t *ids, uint32_t first_id, hipStream_t st) {
    if (!B.n_work) return;
    if (ids)
        hipLaunchKernelGGL(k_pair_emit<true>, dim3(grid_for(B.n_work)), dim3(FD_WAVE), 0, st, B, C, seg_off, cursor, keys, ids, first_id);
    else
        hipLaunchKernelGGL(k_pair_emit<false>, dim3(grid_for(B.n_work)), dim3(FD_WAVE), 0, st, B, C, seg_off, cursor, keys, ids, first_id);
}
void fd_launch_frames(const fd_batch_view &B, uint64_t n_res, void *frames, hipStream_t st) {
    if (!n_res) return;
    hipLaunchKernelGGL(k_frames, dim3((unsigned)((n_res + 255) / 256)), dim3(256), 0, st, B, (uint32_t)n_res, (fd_frame *)frames);
}
void fd_launch_pair_count2(const fd_batch_view &B, const fd_hash_consts &C, uint32_t *counts, hipStream_t st) {
    if (!B.n_work) return;
    hipLaunchKernelGGL(k_pair_count2, dim3(grid_for(B.n_work)), dim3(FD_WAVE), 0, st, B, C, counts);
}
void fd_launch_pair_emit2(const fd_batch_view &B, const void *frames, const fd_hash_consts &C, const uint64_t *seg_off, uint32_t *cursor,
                          uint32_t *keys, void *ids, bool ids16, uint32_t first_id, hipStream_t st) {
    if (!B.n_work) return;
    dim3 g(grid_for(B.n_work)), b(FD_WAVE);
    const fd_frame *F = (const fd_frame *)frames;
    if (C.use_tab >= 2 && ids16) hipLaunchKernelGGL((k_pair_emit2<2, true, false>), g, b, 0, st, B, F, C, seg_off, cursor, keys, ids, first_id, (const uint64_t *)nullptr);
    else if (C.use_tab >= 2) hipLaunchKernelGGL((k_pair_emit2<2, false, false>), g, b, 0, st, B, F, C, seg_off, cursor, keys, ids, first_id, (const uint64_t *)nullptr);
    else if (C.use_tab && ids16) hipLaunchKernelGGL((k_pair_emit2<1, true, false>), g, b, 0, st, B, F, C, seg_off, cursor, keys, ids, first_id, (const uint64_t *)nullptr);
    else if (C.use_tab) hipLaunchKernelGGL((k_pair_emit2<1, false, false>), g, b, 0, st, B, F, C, seg_off, cursor, keys, ids, first_id, (const uint64_t *)nullptr);
    else if (ids16) hipLaunchKernelGGL((k_pair_emit2<0, true, false>), g, b, 0, st, B, F, C, seg_off, cursor, keys, ids, first_id, (const uint64_t *)nullptr);
    else hipLaunchKernelGGL((k_pair_emit2<0, false, false>), g, b, 0, st, B, F, C, seg_off, cursor, keys, ids, first_id, (const uint64_t *)nullptr);
}
// the MSD build (6-byte elements): B = the permuted view (ca_xyz / hash_ok / aa = the arrays k_frames_perm wrote), counts / seg_off = [40][n_work]
void fd_launch_frames_perm(const fd_batch_view &B, float *ca_perm, uint8_t *ok_perm, uint8_t *aa_perm, uint32_t *src_perm, unsigned long long *wide_flag, hipStream_t st) {
    if (!B.n_struct) return;
    hipLaunchKernelGGL(k_frames_perm, dim3(B.n_struct), dim3(256), 0, st, B, ca_perm, ok_perm, aa_perm, src_perm, wide_flag);
}
// n_xyz / cb_xyz: the batch's own arrays (chain order), src_perm: what k_frames_perm wrote; the kernel fills frames (permuted order) and, where
// masks is not null, the mask table ([B.wi_col[n_work]] words) that fd_launch_pair_emit_msd then takes
void fd_launch_pair_count_msd(const fd_batch_view &B, const fd_hash_consts &C, const float *n_xyz, const float *cb_xyz, const uint32_t *src_perm, void *frames,
                              uint32_t *counts, uint64_t *masks, hipStream_t st) {
    if (!B.n_work) return;
    dim3 g(grid_for(B.n_work)), b(FD_WAVE);
    if (masks) hipLaunchKernelGGL(k_pair_count_msd<true>, g, b, 0, st, B, C, n_xyz, cb_xyz, src_perm, (fd_frame *)frames, counts, masks);
    else hipLaunchKernelGGL(k_pair_count_msd<false>, g, b, 0, st, B, C, n_xyz, cb_xyz, src_perm, (fd_frame *)frames, counts, (uint64_t *)nullptr);
}
// masks: the table this call's count pass stored, or null: the kernel then runs the distance filter itself
void fd_launch_pair_emit_msd(const fd_batch_view &B, const void *frames, const fd_hash_consts &C, const uint64_t *seg_off, uint32_t *keys,
                             uint16_t *ids, const uint64_t *masks, hipStream_t st) {
    if (!B.n_work) return;
    dim3 g(grid_for(B.n_work)), b(FD_WAVE);
    const fd_frame *F = (const fd_frame *)frames;
    const uint64_t *no = nullptr;
    if (C.use_tab == 3 && masks) hipLaunchKernelGGL((k_pair_emit2<2, true, true, true, true>), g, b, 0, st, B, F, C, seg_off, (uint32_t *)nullptr, keys, (void *)ids, 0u, masks);
    else if (C.use_tab == 3) hipLaunchKernelGGL((k_pair_emit2<2, true, true, true>), g, b, 0, st, B, F, C, seg_off, (uint32_t *)nullptr, keys, (void *)ids, 0u, no);      // + squared-distance table
    else if (C.use_tab == 2) hipLaunchKernelGGL((k_pair_emit2<2, true, true>), g, b, 0, st, B, F, C, seg_off, (uint32_t *)nullptr, keys, (void *)ids, 0u, no);
    else if (C.use_tab) hipLaunchKernelGGL((k_pair_emit2<1, true, true>), g, b, 0, st, B, F, C, seg_off, (uint32_t *)nullptr, keys, (void *)ids, 0u, no);
    else hipLaunchKernelGGL((k_pair_emit2<0, true, true>), g, b, 0, st, B, F, C, seg_off, (uint32_t *)nullptr, keys, (void *)ids, 0u, no);
}
void fd_launch_row_count(const fd_batch_view &B, const fd_hash_consts &C, uint32_t *row_cnt, float cutoff, hipStream_t st) {
    if (!B.n_work) return;
    hipLaunchKernelGGL(k_row_count, dim3(grid_for(B.n_work)), dim3(FD_WAVE), 0, st, B, C, row_cnt, cutoff);
}
void fd_launch_row_emit(const fd_batch_view &B, const fd_hash_consts &C, const uint64_t *row_off, uint32_t *keys, float cutoff, uint32_t *ids,
                        uint32_t first_id, hipStream_t st, int ids_partner) {
    if (!B.n_work) return;
    hipLaunchKernelGGL(k_row_emit, dim3(grid_for(B.n_work)), dim3(FD_WAVE), 0, st, B, C, row_off, keys, cutoff, ids, first_id, ids_partner);
}
}
