// k_index.hip — posting-list encoding from the sorted (hash, id) stream.
//
// Replaces count_single_entry / allocate_entries / add_single_entry /
// wrapup_offset_and_save_entries / prune_to_sparse of the reference
// (src/index/indextable.rs:88-105, 204-237, 171-202, 239-295, codec :397-418):
//   * duplicates (same hash, same id — the reference's per-structure dedup, mod.rs:343-345) drop out,
//   * first id of a list is absolute, the rest are deltas, each LEB128 (the format of fd_postings.h),
//   * lists are laid out in ascending hash order; only non-empty hashes are kept (sparse form):
//     hashes[H], offsets[H+1] with offsets[k] = first byte of list k, offsets[H] = total bytes.
// Two streaming passes over the sorted pairs (sizes, then write), HBM-bound.
//
// Precondition of the MSD stream (codec 2, B24 below): inside every one of the forty buckets the u16 plane (hash[23:8]) is non-decreasing.  The
// segmented sort guarantees it (fd_radix_sort_pairs16_seg, k_sort.hip, with the digit order of the build, fd_api_build.hip: hash[7:0], then the u16
// plane's low byte, then its high byte LAST, each pass stable), and fdgpu_debug_encode_stream_b24 checks it of a caller's stream.  Both passes
// rely on it: a tile of ENC_TILE elements that lies in one bucket, predecessor element included, and whose two end elements carry the same u16
// value holds that value everywhere, so such a tile reads two elements of the plane and not its 4 KB (enc_b24::cst).  The two passes take the
// same decision for a tile: same predicate, same inputs.  A constant tile that is full and not tile 0 is also classified from the u32 key word alone
// (enc_classify_const: 98 % of a protein build's tiles; again one predicate for both passes).  Codecs 0 and 1 have no such path: their second plane is the id.
#include "fd_device.h"
#include "fd_postings.h"

#define ENC_THREADS 256
#define ENC_ITEMS 8
#define ENC_TILE (ENC_THREADS * ENC_ITEMS)

struct enc_item { uint32_t len; uint32_t head; uint32_t delta; uint32_t hash; };

// three element encodings of the sorted stream:
//   V = uint32_t      : keys[p] = hash,                      vals[p] = structure id
//   V = uint16_t      : keys[p] = hash << 2 | (local >> 16), vals[p] = local & 0xffff, id = first_id + local  (6-byte elements, 2^18 structures)
//   V = uint16_t, B24 : keys[p] = hash[7:0] << 24 | local, vals[p] = hash[23:8]  — the MSD build's stream (digit planes: k_sort.hip): the top six
//                       hash bits ARE the bucket the position p lies in (bucket b = [seg_off[b * stride], seg_off[(b + 1) * stride]), stride = the build's work items), the two planes keep
//                       the other 24 and the whole local id (2^24 structures): hash = bucket << 24 | val << 8 | key >> 24, id = first_id + (key & 0xffffff)
template <typename V> struct enc_codec;
template <> struct enc_codec<uint32_t> {
    static __device__ __forceinline__ uint32_t hash(uint32_t k) { return k; }
    static __device__ __forceinline__ uint32_t id(uint32_t, uint32_t v, uint32_t) { return v; }
};
template <> struct enc_codec<uint16_t> {
    static __device__ __forceinline__ uint32_t hash(uint32_t k) { return k >> 2; }
    static __device__ __forceinline__ uint32_t id(uint32_t k, uint16_t v, uint32_t first_id) { return first_id + (((k & 3u) << 16) | v); }
};

#define ENC_BUCKETS 40u
struct enc_b24 {              // B24: where the forty buckets start (bo[0..40], compact copy of seg_off[b * stride]) and the tile's first / last bucket
    const uint64_t *bo;
    uint32_t b0, b1;
    bool cst;                 // the tile and its predecessor element hold ONE u16 value, `ev` (workgroup-uniform; see the precondition above)
    uint32_t ev;
    uint32_t wpk;             // the key word in front of the WAVE's first element: lane 0's predecessor (wave-uniform; meaningless where there is none)
    __device__ __forceinline__ uint32_t at(uint64_t p) const { uint32_t b = b0; while (b < b1 && p >= bo[b + 1]) ++b; return b; }      // tiles on a boundary only
};
// What a wave reads to classify its tile, per wave, no LDS and no barrier: lane l holds bo[l], every lane the u16 values at the tile's two ends (tp =
// the predecessor of its first element, t1 = its last valid one).  Issued BEFORE the tile's key loads: the memory counter retires loads in issue
// order, so enc_b24_setup's wait for these three leaves the key loads in flight, where behind them it would be the wait for the keys as well.
// With them, and for the same reason not behind the keys: the key word in front of the wave's first element (index clamped into the stream).
struct enc_b24_raw { uint64_t o; uint32_t e0, e1, wpk; };
__device__ __forceinline__ enc_b24_raw enc_b24_fetch(const uint32_t *__restrict__ keys, const uint64_t *__restrict__ bo, const uint16_t *__restrict__ vals, uint64_t n, bool full) {
    const uint64_t t0 = (uint64_t)blockIdx.x * (256 * 8);
    const uint64_t t1 = (t0 + 256 * 8 < n ? t0 + 256 * 8 : n) - 1;
    const uint64_t tp = t0 ? t0 - 1 : 0;
    const uint32_t lane = threadIdx.x & 63;
    enc_b24_raw R;
    R.o = lane >= 1 && lane <= ENC_BUCKETS ? bo[lane] : ~0ull;
    R.e0 = vals[tp];
    R.e1 = vals[t1];
    const uint64_t w0 = t0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (64u * 8u);
    const uint64_t wq = full || w0 < n ? w0 : n;      // full: the tile lies inside the stream; n >= 1
    R.wpk = keys[wq ? wq - 1 : 0];
    return R;
}
__device__ __forceinline__ enc_b24 enc_b24_setup(const uint64_t *__restrict__ bo, uint64_t n, const enc_b24_raw &R) {
    const uint64_t t0 = (uint64_t)blockIdx.x * (256 * 8);
    const uint64_t t1 = (t0 + 256 * 8 < n ? t0 + 256 * 8 : n) - 1;
    const uint64_t tp = t0 ? t0 - 1 : 0;      // the predecessor of the tile's first element is classified too
    const uint32_t lane = threadIdx.x & 63;
    const bool in = lane >= 1 && lane <= ENC_BUCKETS;
    enc_b24 K;
    K.bo = bo;
    K.b0 = (uint32_t)__popcll(__ballot(in && R.o <= tp));      // buckets 1..40 that start at or before p: the bucket p lies in
    K.b1 = (uint32_t)__popcll(__ballot(in && R.o <= t1));
    if (K.b0 >= ENC_BUCKETS) K.b0 = ENC_BUCKETS - 1;
    if (K.b1 >= ENC_BUCKETS) K.b1 = ENC_BUCKETS - 1;
    // every lane loaded the same two elements: as scalars, so that the branches on `cst` are uniform branches and not exec masks
    // (both read before the comparison: behind a short-circuit the compiler moves the load of e0 there too, one more round trip)
    const uint32_t e0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)R.e0);
    K.ev = (uint32_t)__builtin_amdgcn_readfirstlane((int)R.e1);
    K.cst = (K.b0 == K.b1) & (e0 == K.ev);
    K.wpk = R.wpk;
    return K;
}
__global__ void k_enc_bucket_starts(const uint64_t *__restrict__ seg_off, uint64_t S, uint64_t *__restrict__ bo) {
    if (threadIdx.x <= ENC_BUCKETS) bo[threadIdx.x] = seg_off[(uint64_t)threadIdx.x * S];
}

// The two ways a thread gets its ENC_ITEMS (= 8) consecutive elements: 16-byte loads, or guarded loads per element at the stream's end.  B24: each
// is ONE straight run — edge loads, key loads, the decision, the u16 plane if the tile is not constant — and enc_load_classify branches between
// the two whole runs.  With the branch around the key loads alone, both sides met again before the decision, and there the compiler counts
// the loads behind the edge loads by the side with the fewest (the guarded ones count as none): it waited for the keys before it looked at the
// tile's ends.
template <typename V, bool B24>
__device__ __forceinline__ enc_b24 enc_load_full(const uint32_t *__restrict__ keys, const V *__restrict__ ids, uint64_t n, uint64_t base,
                                                 const uint64_t *__restrict__ bo, uint32_t *k, uint32_t *v) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    enc_b24_raw R = {};
    if (B24) R = enc_b24_fetch(keys, bo, (const uint16_t *)ids, n, true);
    const u32x4 *kp = reinterpret_cast<const u32x4 *>(keys + base);
    u32x4 a = __builtin_nontemporal_load(&kp[0]), b = __builtin_nontemporal_load(&kp[1]);
    k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w; k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
    enc_b24 K = {};
    if (B24) K = enc_b24_setup(bo, n, R);
    if (B24 && K.cst) {      // workgroup-uniform: nothing to load, and enc_load_classify fills v with K.ev where it goes the general way
    } else if (sizeof(V) == 2) {
        u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(ids + base));
        v[0] = w.x & 0xffffu; v[1] = w.x >> 16; v[2] = w.y & 0xffffu; v[3] = w.y >> 16;
        v[4] = w.z & 0xffffu; v[5] = w.z >> 16; v[6] = w.w & 0xffffu; v[7] = w.w >> 16;
    } else {
        const u32x4 *vp = reinterpret_cast<const u32x4 *>(ids + base);
        u32x4 c = __builtin_nontemporal_load(&vp[0]), d = __builtin_nontemporal_load(&vp[1]);
        v[0] = c.x; v[1] = c.y; v[2] = c.z; v[3] = c.w; v[4] = d.x; v[5] = d.y; v[6] = d.z; v[7] = d.w;
    }
    return K;
}
template <typename V, bool B24>
__device__ __forceinline__ enc_b24 enc_load_tail(const uint32_t *__restrict__ keys, const V *__restrict__ ids, uint64_t n, uint64_t base,
                                                 const uint64_t *__restrict__ bo, uint32_t *k, uint32_t *v) {
    enc_b24 K = {};
    if (B24) K = enc_b24_setup(bo, n, enc_b24_fetch(keys, bo, (const uint16_t *)ids, n, false));
#pragma unroll
    for (int j = 0; j < ENC_ITEMS; ++j) {
        uint64_t p = base + j;
        k[j] = p < n ? keys[p] : 0u;
        v[j] = B24 && K.cst ? K.ev : p < n ? (uint32_t)ids[p] : 0u;
    }
    return K;
}

// A full constant tile behind tile 0 (enc_load_classify's fast path; 98 % of a protein build's tiles): bucket and u16 value are the tile's, so the
// key word alone tells heads, repeats and deltas (fd_postings.h: fd_const_*), no element lies beyond n, and every element has a predecessor —
// the previous item, the neighbouring lane's last one, or for lane 0 keys[base - 1] (enc_b24::wpk), which belongs to the same constant run by the
// definition of `cst`.  Every element is classified as a delta; what a list head needs beyond that (its id, its hash, the id in front of the thread) is made
// behind one test of the wavefront's heads — one element in ~700 is a head — or, in the tile that ends the stream, for its last-id store.
// -> ENC_FAST if the wavefront holds no head (it[].head, it[].hash are 0 and *pred_id is not written), else ENC_FAST_HEADS
enum { ENC_GENERAL = 0, ENC_FAST = 1, ENC_FAST_HEADS = 2 };
__device__ __forceinline__ int enc_classify_const(uint64_t n, uint32_t first_id, const enc_b24 &K,
                                                  const uint32_t *k, enc_item *it, uint32_t *bytes, uint32_t *heads, uint32_t *pred_id) {
    // the lane below's last key in one DPP move (wave_shr:1); lane 0 has no lane below and keeps the move's old value, the wave's predecessor
    const uint32_t pk0 = (uint32_t)__builtin_amdgcn_update_dpp((int)K.wpk, (int)k[ENC_ITEMS - 1], 0x138, 0xf, 0xf, false);
    uint32_t pk = pk0, hx = 0;
#pragma unroll
    for (int j = 0; j < ENC_ITEMS; ++j) {
        hx |= k[j] ^ pk;
        it[j].delta = fd_const_delta(k[j], pk, &it[j].len);
        it[j].head = 0u; it[j].hash = 0u;
        pk = k[j];
    }
    int path = ENC_FAST;
    *heads = 0u;
    const bool ends_stream = ((uint64_t)blockIdx.x + 1) * ENC_TILE == n;      // workgroup-uniform
    if (__ballot((hx >> 24) != 0u) != 0ull || ends_stream) {      // wave-uniform
        path = ENC_FAST_HEADS;
        const uint32_t hash_hi = K.b0 << 24 | K.ev << 8;
        uint32_t nh = 0;
        pk = pk0;
#pragma unroll
        for (int j = 0; j < ENC_ITEMS; ++j) {
            if (fd_const_is_head(k[j], pk)) {
                it[j].delta = fd_const_head(k[j], first_id, &it[j].len);
                it[j].head = 1u; it[j].hash = hash_hi | k[j] >> 24;
                ++nh;
            }
            pk = k[j];
        }
        *heads = nh;
        if (pred_id) *pred_id = first_id + (pk0 & 0xffffffu);
    }
    uint32_t b = 0;
#pragma unroll
    for (int j = 0; j < ENC_ITEMS; ++j) b += it[j].len;
    *bytes = b;
    return path;
}

// Loads the thread's elements and classifies them; the predecessor of the thread's first element comes from the neighbouring lane (shuffle)
// or, for lane 0 of a wave, from memory.  B24: a constant tile (enc_b24::cst) reads nothing of the u16 plane but its two end elements, and if it is
// full and not tile 0 it takes enc_classify_const — a workgroup-uniform decision, and the one expression for both passes.  Every other tile
// (tile 0, whose element 0 has no predecessor; the stream's partial last tile; a tile on a bucket boundary or with a change of the u16 value)
// goes the general way.  -> the path taken, the thread's bytes and heads; an element that writes nothing (a repeat, one beyond n) has len 0, delta 0.
template <typename V, bool B24>
__device__ __forceinline__ int enc_load_classify(const uint32_t *__restrict__ keys, const V *__restrict__ ids, uint64_t n, uint64_t base,
                                                 uint32_t first_id, enc_item *it, const uint64_t *__restrict__ bo, uint32_t *bytes, uint32_t *heads,
                                                 uint32_t *pred_id = nullptr) {
    uint32_t k[ENC_ITEMS], v[ENC_ITEMS];
    // B24: by the tile and not by the thread, so that the whole workgroup goes one way (enc_b24_setup holds wave-wide ballots)
    const bool full = B24 ? ((uint64_t)blockIdx.x + 1) * ENC_TILE <= n : base + ENC_ITEMS <= n;
    const enc_b24 K = full ? enc_load_full<V, B24>(keys, ids, n, base, bo, k, v) : enc_load_tail<V, B24>(keys, ids, n, base, bo, k, v);
    if (B24 && full && K.cst && blockIdx.x != 0) return enc_classify_const(n, first_id, K, k, it, bytes, heads, pred_id);
    if (B24 && full && K.cst) {
#pragma unroll
        for (int j = 0; j < ENC_ITEMS; ++j) v[j] = K.ev;
    }
    // predecessor of element 0
    uint32_t pk = __shfl_up(k[ENC_ITEMS - 1], 1, FD_WAVE), pv = __shfl_up(v[ENC_ITEMS - 1], 1, FD_WAVE);
    if ((threadIdx.x & 63) == 0 && base > 0 && base < n) { pk = B24 ? K.wpk : keys[base - 1]; pv = B24 && K.cst ? K.ev : (uint32_t)ids[base - 1]; }
    uint32_t ph, pid;
    uint32_t hb[ENC_ITEMS];      // B24: the items' bucket << 24 — one value for the whole tile unless it lies on one of the 40 boundaries
    if (B24) {
        uint32_t pb = K.b0;
#pragma unroll
        for (int j = 0; j < ENC_ITEMS; ++j) hb[j] = K.b0 << 24;
        if (K.b0 != K.b1) {      // block-uniform
            if (base) pb = K.at(base - 1);
#pragma unroll
            for (int j = 0; j < ENC_ITEMS; ++j) if (base + j < n) hb[j] = K.at(base + j) << 24;
        }
        ph = pb << 24 | pv << 8 | pk >> 24; pid = first_id + (pk & 0xffffffu);
    } else { ph = enc_codec<V>::hash(pk); pid = enc_codec<V>::id(pk, (V)pv, first_id); }
    if (pred_id) *pred_id = pid;     // id of the element before the thread's first one (undefined for element 0)
    bool have_prev = base > 0;
    uint32_t b = 0, nh = 0;
#pragma unroll
    for (int j = 0; j < ENC_ITEMS; ++j) {
        uint64_t p = base + j;
        uint32_t h, id;
        if (B24) { h = hb[j] | v[j] << 8 | k[j] >> 24; id = first_id + (k[j] & 0xffffffu); }
        else { h = enc_codec<V>::hash(k[j]); id = enc_codec<V>::id(k[j], (V)v[j], first_id); }
        bool in = p < n;
        bool head = !have_prev || ph != h;
        bool dup = !head && pid == id;
        it[j].hash = h;
        it[j].head = (in && head) ? 1u : 0u;
        it[j].delta = !in ? 0u : head ? id : id - pid;
        it[j].len = (!in || dup) ? 0u : fd_varint_len(it[j].delta);
        b += it[j].len; nh += it[j].head;
        ph = h; pid = id; have_prev = true;
    }
    *bytes = b; *heads = nh;
    return ENC_GENERAL;
}

// inclusive prefix sum over the wavefront in six DPP adds (k_qtile.h: qt_wave_incl): row_shr 1/2/4/8 inside the rows of 16 lanes, then row_bcast:15 /
// row_bcast:31 carry the row totals across; lane 63 ends with the wave's total
__device__ __forceinline__ uint32_t enc_wave_incl(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t v) {
    uint32_t lane = threadIdx.x & 63;
    for (int off = 1; off < 64; off <<= 1) {
        uint64_t t = __shfl_up(v, off, FD_WAVE);
        if ((int)lane >= off) v += t;
    }
    return v;
}
// packs (bytes << 32 | entries... ) no: two independent u64 scans share the shuffles poorly; bytes per
// tile < 2^16 and heads per tile < 2^12, so both fit one u32 pair packed in a u64: hi = bytes, lo = heads.
__device__ __forceinline__ uint64_t block_excl_scan_packed(uint64_t v, uint64_t *sm, uint64_t *total) {
    uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint64_t inc = wave_incl_scan64(v);
    if (lane == 63) sm[wid] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < ENC_THREADS / 64; ++w) {
        uint64_t t = sm[w];
        if (w < wid) base += t;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return inc - v + base;
}

// pass 1: per-tile (bytes, heads, postings) sums
template <typename V, bool B24>
__global__ __launch_bounds__(ENC_THREADS) void k_enc_sizes(const uint32_t *__restrict__ keys, const V *__restrict__ ids, uint64_t n, uint32_t first_id,
                                                           uint32_t *__restrict__ tile_bytes, uint32_t *__restrict__ tile_heads,
                                                           uint32_t *__restrict__ tile_posts, const uint64_t *__restrict__ bo) {
    __shared__ uint64_t sm[ENC_THREADS / 64];
    uint64_t base = (uint64_t)blockIdx.x * ENC_TILE + (uint64_t)threadIdx.x * ENC_ITEMS;
    uint32_t bytes = 0, heads = 0, posts = 0;
    enc_item it[ENC_ITEMS];
    const int path = enc_load_classify<V, B24>(keys, ids, n, base, first_id, it, bo, &bytes, &heads);
    if (B24 && path != ENC_GENERAL) {      // workgroup-uniform.  Totals, not a scan: postings from the popcounts of the items' ballots (scalar), bytes and heads by one wave sum
        __shared__ uint32_t sw[ENC_THREADS / 64][3];
        uint32_t wp = 0;
#pragma unroll
        for (int k = 0; k < ENC_ITEMS; ++k) wp += (uint32_t)__popcll(__ballot(it[k].len != 0u));
        const uint32_t mine = bytes << 16 | heads;      // below 2^16 each in a wave; heads are 0 but in a wavefront of ENC_FAST_HEADS
        const uint32_t wbh = (uint32_t)__builtin_amdgcn_readlane((int)enc_wave_incl(mine), 63);
        const uint32_t wb = wbh >> 16, wh = wbh & 0xffffu;
        if ((threadIdx.x & 63) == 0) { uint32_t *w = sw[threadIdx.x >> 6]; w[0] = wb; w[1] = wh; w[2] = wp; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t t[3] = {0u, 0u, 0u};
            for (int w = 0; w < ENC_THREADS / 64; ++w) for (int q = 0; q < 3; ++q) t[q] += sw[w][q];
            tile_bytes[blockIdx.x] = t[0];
            tile_heads[blockIdx.x] = t[1];
            tile_posts[blockIdx.x] = t[2];
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < ENC_ITEMS; ++k) posts += it[k].len ? 1u : 0u;
    uint64_t tot;
    block_excl_scan_packed(((uint64_t)bytes << 32) | heads, sm, &tot);
    // postings: separate reduction
    uint32_t pw = posts;
    for (int off = 32; off > 0; off >>= 1) pw += __shfl_down(pw, off, FD_WAVE);
    __shared__ uint32_t pp[ENC_THREADS / 64];
    if ((threadIdx.x & 63) == 0) pp[threadIdx.x >> 6] = pw;
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_bytes[blockIdx.x] = (uint32_t)(tot >> 32);
        tile_heads[blockIdx.x] = (uint32_t)tot;
        uint32_t t = 0;
        for (int w = 0; w < ENC_THREADS / 64; ++w) t += pp[w];
        tile_posts[blockIdx.x] = t;
    }
}

// pass 2: write varint bytes, sparse hashes and list start offsets
#define ENC_LDS_BYTES (ENC_TILE * 5 + 32)
// a tile of ENC_TILE five-byte varints behind the largest alignment shift, rounded up to the dword the varint writer ORs into and to the
// 16 bytes the zeroing and the write-out move at a time
static_assert(ENC_LDS_BYTES % 16 == 0 && (ENC_TILE * 5 + 15 + 15) / 16 * 16 <= ENC_LDS_BYTES, "s_bytes: a full tile of five-byte varints must fit");
template <typename V, bool B24>
__global__ __launch_bounds__(ENC_THREADS) void k_enc_write(const uint32_t *__restrict__ keys, const V *__restrict__ ids, uint64_t n, uint32_t first_id,
                                                           const uint64_t *__restrict__ tile_byte_off, const uint64_t *__restrict__ tile_head_off,
                                                           uint8_t *__restrict__ value, uint32_t *__restrict__ hashes, uint64_t *__restrict__ offsets,
                                                           uint32_t *__restrict__ last_ids, const uint64_t *__restrict__ bo) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    __shared__ uint32_t sm[ENC_THREADS / 64];
    // varint bytes of the tile are assembled in LDS (pre-shifted by the global misalignment) and leave as
    // 16-byte stores instead of one global byte store per byte
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[ENC_LDS_BYTES];
    uint32_t *const s_dw = reinterpret_cast<uint32_t *>(s_bytes);
    const uint64_t base = (uint64_t)blockIdx.x * ENC_TILE + (uint64_t)threadIdx.x * ENC_ITEMS;
    enc_item it[ENC_ITEMS];
    uint32_t bytes = 0, heads = 0;
    uint32_t run_id = 0;   // id of the element before item k (for the per-list last ids)
    const int path = enc_load_classify<V, B24>(keys, ids, n, base, first_id, it, bo, &bytes, &heads, &run_id);
    // one scan for both: a tile holds at most ENC_TILE * 5 bytes and ENC_TILE heads, 16 bits each (hi = bytes, lo = heads).  The tile's length is
    // known after the scan's first barrier, so the bytes the tile will use are zeroed between the two (the writer below ORs into them)
    static_assert(ENC_TILE * 5 < (1 << 16), "bytes and heads of a tile are scanned as the halves of one u32");
    const uint32_t mine = bytes << 16 | heads;
    const uint32_t inc = enc_wave_incl(mine);
    if ((threadIdx.x & 63) == 63) sm[threadIdx.x >> 6] = inc;
    const uint64_t tile_b0 = tile_byte_off[blockIdx.x];
    const uint32_t shift = (uint32_t)(tile_b0 & 15ull);
    __syncthreads();
    uint32_t ex = inc - mine, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < ENC_THREADS / 64; ++w) {
        const uint32_t t = sm[w];
        if (w < (threadIdx.x >> 6)) ex += t;
        tot += t;
    }
    const uint32_t tile_len = tot >> 16;
    const uint32_t end = shift + tile_len;                 // LDS range [shift, end) holds the tile's bytes
    for (uint32_t c = threadIdx.x * 16; c < end; c += ENC_THREADS * 16) *reinterpret_cast<u32x4 *>(s_bytes + c) = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    const uint32_t lo = shift + (ex >> 16);                // LDS position of this thread's first byte
    // list heads and the stream's last element: one item in ~700 of a protein index, so everything they need (64-bit offsets, the running id)
    // stays out of the byte path; a wavefront of a constant tile that holds neither (ENC_FAST) does not even test for them
    if (path != ENC_FAST) {      // wave-uniform
        const bool tail = base < n && n - base <= ENC_ITEMS;
        if (heads | (tail ? 1u : 0u)) {
            uint64_t hoff = tile_head_off[blockIdx.x] + (ex & 0xffffu);
            const uint64_t boff = tile_b0 + (ex >> 16);
            const uint32_t k_last = tail ? (uint32_t)(n - base) - 1u : ENC_ITEMS;
            uint32_t pre = 0;
#pragma unroll
            for (uint32_t k = 0; k < ENC_ITEMS; ++k) {
                if (it[k].head) {
                    hashes[hoff] = it[k].hash;
                    offsets[hoff] = boff + pre;
                    if (hoff) last_ids[hoff - 1] = run_id;            // the list before this head ends on the preceding element
                    ++hoff;
                }
                run_id = it[k].head ? it[k].delta : run_id + it[k].delta;
                if (k == k_last) last_ids[hoff - 1] = run_id;         // last element: its own id
                pre += it[k].len;
            }
        }
    }
    // The thread's varints are adjacent in the output: each is packed in a register (fd_varint_pack) and appended to a 64-bit accumulator that
    // holds the bytes of the dword being filled (at most 3 pending + 5 new).  Every item ORs the accumulator's low dword into LDS — complete or
    // not: the bits are final, the next item's OR adds the rest — so the only branch is the second dword a five-byte varint can complete.  An OR
    // and not a store, because a thread's first and last dwords also hold its neighbours' bytes.  A thread without bytes ORs zeros at its position
    // (a repeat or an element beyond n has len 0 AND delta 0: enc_load_classify).
    uint32_t pos = lo;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < ENC_ITEMS; ++k) {
        const uint32_t len = it[k].len;
        acc |= fd_varint_pack(it[k].delta, len) << (8u * (pos & 3u));
        atomicOr(&s_dw[pos >> 2], (uint32_t)acc);
        const uint32_t npos = pos + len;
        const uint32_t filled = (npos >> 2) - (pos >> 2);          // dwords completed by this item: 0, 1, or 2
        if (filled > 1) { atomicOr(&s_dw[(pos >> 2) + 1], (uint32_t)(acc >> 32)); acc = 0; }
        else acc = filled ? acc >> 32 : acc;
        pos = npos;
    }
    atomicOr(&s_dw[pos >> 2], (uint32_t)acc);      // pos <= end: inside s_bytes (static_assert above)
    __syncthreads();
    uint8_t *gbase = value + (tile_b0 - shift);            // 16-byte aligned (value comes from hipMalloc)
    for (uint32_t c = threadIdx.x * 16; c < end; c += ENC_THREADS * 16) {
        if (c >= shift && c + 16 <= end) {
            *reinterpret_cast<u32x4 *>(gbase + c) = *reinterpret_cast<const u32x4 *>(s_bytes + c);
        } else {
            for (uint32_t b = c < shift ? shift : c; b < c + 16 && b < end; ++b) gbase[b] = s_bytes[b];
        }
    }
}

__global__ void k_set_u64(uint64_t *dst, uint64_t idx, const uint64_t *src) { dst[idx] = src[0]; }

uint32_t fd_enc_num_tiles(uint64_t n) { return (uint32_t)((n + ENC_TILE - 1) / ENC_TILE); }
// codec: 0 = (u32 hash, u32 id), 1 = 6-byte elements of the structure-major stream, 2 = 6-byte elements of the MSD stream (seg_off = its [40][S]
// table, S here = the table's stride: the build's work items, bo = 41 words of scratch that receive the bucket starts; fd_launch_enc_write reads them again)
void fd_launch_enc_sizes(const uint32_t *keys, const void *ids, int codec, uint32_t first_id, uint64_t n, uint32_t *tb, uint32_t *th, uint32_t *tp,
                         const uint64_t *seg_off, uint64_t S, uint64_t *bo, hipStream_t st) {
    if (!n) return;
    const dim3 g(fd_enc_num_tiles(n)), t(ENC_THREADS);
    if (codec == 2) hipLaunchKernelGGL(k_enc_bucket_starts, dim3(1), dim3(64), 0, st, seg_off, S, bo);
    if (codec == 2) hipLaunchKernelGGL((k_enc_sizes<uint16_t, true>), g, t, 0, st, keys, (const uint16_t *)ids, n, first_id, tb, th, tp, bo);
    else if (codec == 1) hipLaunchKernelGGL((k_enc_sizes<uint16_t, false>), g, t, 0, st, keys, (const uint16_t *)ids, n, first_id, tb, th, tp, bo);
    else hipLaunchKernelGGL((k_enc_sizes<uint32_t, false>), g, t, 0, st, keys, (const uint32_t *)ids, n, first_id, tb, th, tp, bo);
}
void fd_launch_enc_write(const uint32_t *keys, const void *ids, int codec, uint32_t first_id, uint64_t n, const uint64_t *tbo, const uint64_t *tho,
                         uint8_t *value, uint32_t *hashes, uint64_t *offsets, uint32_t *last_ids, const uint64_t *total_bytes_dev, uint64_t H,
                         const uint64_t *bo, hipStream_t st) {
    if (n) {
        const dim3 g(fd_enc_num_tiles(n)), t(ENC_THREADS);
        if (codec == 2) hipLaunchKernelGGL((k_enc_write<uint16_t, true>), g, t, 0, st, keys, (const uint16_t *)ids, n, first_id, tbo, tho, value, hashes, offsets, last_ids, bo);
        else if (codec == 1) hipLaunchKernelGGL((k_enc_write<uint16_t, false>), g, t, 0, st, keys, (const uint16_t *)ids, n, first_id, tbo, tho, value, hashes, offsets, last_ids, bo);
        else hipLaunchKernelGGL((k_enc_write<uint32_t, false>), g, t, 0, st, keys, (const uint32_t *)ids, n, first_id, tbo, tho, value, hashes, offsets, last_ids, bo);
    }
    hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, st, offsets, H, total_bytes_dev);
}
