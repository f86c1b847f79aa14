// fd_api_build.hip — C ABI of libfdgpu.so, seam S1 and the build half of S2 (include/fdgpu.h): the hashers (fdgpu_hash_batch, fdgpu_hash_batch_rows), the
// index build (fdgpu_index_build) in its three forms, the encoder driver they end in and the two test-only encoder entries (include/fdgpu_debug.h) — the
// orchestration of k_hash.hip, k_sort.hip and k_index.hip.  No kernel lives here.  The index object, export / load / save: fdgpu_api.hip.
#include <stdlib.h>
#include <algorithm>
#include <memory>
#include "fd_api_common.h"

// a call's host arrays belong to these until the success exits release them to the caller
struct ib_free { void operator()(void *p) const { free(p); } };
typedef std::unique_ptr<uint32_t, ib_free> ib_u32_ptr;
typedef std::unique_ptr<uint64_t, ib_free> ib_u64_ptr;

// ---- what the hashers and the build share -----------------------------------------------------------------------------------
// row-major lists: per-residue row counts (WS_MISC0) -> row offsets (WS_MISC1, R + 1 entries) -> *P = their total; one synchronisation.
// stage: the build's timer around count + scan (the hashers report none)
static int row_count_and_scan(fdgpu_ctx *c, const fdgpu_batch *b, const fd_hash_consts &C, float dist_cutoff, uint64_t *P, const char *stage = nullptr) {
    const uint64_t R = b->n_res;
    hipStream_t st = c->stream;
    HIPCHK(c, c->ws[WS_MISC0].ensure((R + 1) * 4));
    HIPCHK(c, c->ws[WS_MISC1].ensure((R + 2) * 8));
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(std::max<uint64_t>(b->n_struct, R)) * 8 + 64));
    HIPCHK(c, c->ws[WS_TOTAL].ensure(64));
    HIPCHK(c, hipMemsetAsync(c->ws[WS_MISC0].p, 0, (R + 1) * 4, st));
    {
        StageTimer t(stage ? c : nullptr, stage, R * 37);
        fd_launch_row_count(b->view(), C, c->ws[WS_MISC0].as<uint32_t>(), dist_cutoff, st);
        fd_exclusive_scan<uint32_t>(c->ws[WS_MISC0].as<uint32_t>(), R, c->ws[WS_MISC1].as<uint64_t>(), c->ws[WS_SCANTMP].as<uint64_t>(),
                                    c->ws[WS_TOTAL].as<uint64_t>(), st);
    }
    HIPCHK(c, hipGetLastError());
    return d2h_u64(c, c->ws[WS_TOTAL].as<uint64_t>(), P);
}

// counts (WS_COUNTS, n entries) -> their exclusive scan (WS_SEGOFF) -> *P = the total; one synchronisation
static int scan_counts(fdgpu_ctx *c, uint64_t n, uint64_t *P) {
    {
        StageTimer t(c, "segment_scan", n * 12);
        fd_exclusive_scan<uint32_t>(c->ws[WS_COUNTS].as<uint32_t>(), n, c->ws[WS_SEGOFF].as<uint64_t>(), c->ws[WS_SCANTMP].as<uint64_t>(),
                                    c->ws[WS_TOTAL].as<uint64_t>(), c->stream);
    }
    HIPCHK(c, hipGetLastError());
    return d2h_u64(c, c->ws[WS_TOTAL].as<uint64_t>(), P);
}
// pair count per structure -> segment offsets (WS_CURSOR cleared for the emit); returns total pairs
static int count_and_scan(fdgpu_ctx *c, const fdgpu_batch *b, const fd_hash_consts &C, uint64_t *P, bool unordered = false) {
    uint64_t S = b->n_struct;
    HIPCHK(c, c->ws[WS_COUNTS].ensure((S + 1) * 4));
    HIPCHK(c, c->ws[WS_CURSOR].ensure((S + 1) * 4));
    HIPCHK(c, c->ws[WS_SEGOFF].ensure((S + 2) * 8));
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(std::max<uint64_t>(S, b->n_res)) * 8 + 64));
    HIPCHK(c, c->ws[WS_TOTAL].ensure(64));
    HIPCHK(c, hipMemsetAsync(c->ws[WS_COUNTS].p, 0, (S + 1) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->ws[WS_CURSOR].p, 0, (S + 1) * 4, c->stream));
    {
        StageTimer t(c, "pair_count", b->n_res * 13);
        if (unordered) fd_launch_pair_count2(b->view(), C, c->ws[WS_COUNTS].as<uint32_t>(), c->stream);
        else fd_launch_pair_count(b->view(), C, c->ws[WS_COUNTS].as<uint32_t>(), c->stream);
    }
    return scan_counts(c, S, P);
}

// the limit on the keys of a call, then the two key and the two payload buffers of a sort of P of them; pointers are taken after the last ensure()
struct ib_keys { uint32_t *ka, *kb; void *ia, *ib; };
static int reserve_keys(fdgpu_ctx *c, uint64_t P, uint64_t max_keys, const char *too_many, size_t id_bytes, ib_keys &K) {
    if (P >= max_keys) FAIL(c, FDGPU_ERANGE, too_many);
    size_t kb = std::max<uint64_t>(P, 1) * 4, ib = std::max<uint64_t>(P, 1) * id_bytes + 16;
    // a call that grows the sort buffers by gigabytes first returns the cached blocks of destroyed indices to the device
    if (kb > c->ws[WS_KEYS_A].cap + ((size_t)1 << 30) || kb > c->ws[WS_KEYS_B].cap + ((size_t)1 << 30)) c->pool_drop();
    HIPCHK(c, c->ws[WS_KEYS_A].ensure(kb));
    HIPCHK(c, c->ws[WS_IDS_A].ensure(ib));
    HIPCHK(c, c->ws[WS_KEYS_B].ensure(kb));
    HIPCHK(c, c->ws[WS_IDS_B].ensure(ib));
    HIPCHK(c, c->ws[WS_GHIST].ensure((size_t)256 * std::max<uint32_t>(fd_rs_num_tiles(P), 1) * 4));
    // 256 digit totals + the chunk sums of the tile-major histogram scan ([tiles / 128][256] u64)
    HIPCHK(c, c->ws[WS_TOT].ensure((256 + (size_t)(fd_rs_num_tiles(P) / 128 + 2) * 256) * 8));
    K.ka = c->ws[WS_KEYS_A].as<uint32_t>(); K.kb = c->ws[WS_KEYS_B].as<uint32_t>();
    K.ia = c->ws[WS_IDS_A].p; K.ib = c->ws[WS_IDS_B].p;
    return FDGPU_OK;
}

// ---- S1 ---------------------------------------------------------------------------------------------------------------
extern "C" int fdgpu_hash_batch(fdgpu_ctx *c, const fdgpu_batch *b, const fd_hash_params *p, int sort_dedup, uint32_t **hashes,
                                uint64_t **hash_off) { FD_LOCK(c);
    if (!c || !b || !p || !hashes || !hash_off) return FDGPU_EINVAL;
    *hashes = nullptr; *hash_off = nullptr;
    if (p->n_multiple_bins) FAIL(c, FDGPU_EINVAL, "hash_batch: multiple_bins is honoured by the index build and the query calls only");
    if (!fd_hash_type_supported(p->hash_type)) FAIL(c, FDGPU_EINVAL, "hash_type: only the encodings over the (d_CA, d_CB, theta, tau1, tau2) descriptor are built (0, 1, 3, 7, 8)");
    reset_timings(c);
    fd_hash_consts C = make_consts(p);
    uint64_t S = b->n_struct, R = b->n_res;
    ib_u64_ptr h_off((uint64_t *)malloc((S + 1) * 8));
    if (!h_off) return FDGPU_ENOMEM;
    hipStream_t st = c->stream;
    int rc;
    if (!sort_dedup) {
        // row-major raw list: per-residue row counts -> row offsets -> ordered emit
        uint64_t P = 0;
        if ((rc = row_count_and_scan(c, b, C, p->dist_cutoff, &P))) return rc;
        HIPCHK(c, c->ws[WS_KEYS_A].ensure(std::max<uint64_t>(P, 1) * 4));
        fd_launch_row_emit(b->view(), C, c->ws[WS_MISC1].as<uint64_t>(), c->ws[WS_KEYS_A].as<uint32_t>(), p->dist_cutoff, nullptr, 0u, st);
        HIPCHK(c, hipGetLastError());
        ib_u32_ptr h((uint32_t *)malloc(std::max<uint64_t>(P, 1) * 4));
        std::vector<uint64_t> row_off(R + 1);
        if (!h) return FDGPU_ENOMEM;
        HIPCHK(c, hipMemcpyAsync(h.get(), c->ws[WS_KEYS_A].p, P * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(row_off.data(), c->ws[WS_MISC1].p, (R + 1) * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        for (uint64_t s = 0; s <= S; ++s) h_off.get()[s] = row_off[b->h_res_off[s]];
        *hashes = h.release(); *hash_off = h_off.release();
        return FDGPU_OK;
    }
    if (fd_own_descriptor(p->hash_type)) FAIL(c, FDGPU_EINVAL, "hash_batch: this encoding is served in the reference's raw order only (sort_dedup = 0)");
    uint64_t P = 0;
    if ((rc = count_and_scan(c, b, C, &P))) return rc;
    ib_keys K;
    if ((rc = reserve_keys(c, P, 0xffffffffull, "more than 2^32 residue pairs in one batch; split the batch", 4, K))) return rc;
    uint32_t *ka = K.ka, *ia = (uint32_t *)K.ia, *kb = K.kb, *ib = (uint32_t *)K.ib;
    fd_launch_pair_emit(b->view(), C, c->ws[WS_SEGOFF].as<uint64_t>(), c->ws[WS_CURSOR].as<uint32_t>(), ka, ia, 0u, st);
    // sort by hash, then (stable) by structure -> (structure, hash) order
    int cur = sort_pairs(c, ka, ia, kb, ib, P, 32);   // all 32 bits: unmasked field overflow can set bits 30-31
    uint32_t *k1 = cur ? kb : ka, *i1 = cur ? ib : ia, *k2 = cur ? ka : kb, *i2 = cur ? ia : ib;
    int id_bits = 1;
    while (id_bits < 32 && (1ull << id_bits) < std::max<uint64_t>(S, 2)) ++id_bits;
    int cur2 = sort_pairs(c, i1, k1, i2, k2, P, id_bits);
    uint32_t *ids_s = cur2 ? i2 : i1, *keys_s = cur2 ? k2 : k1, *spare = cur2 ? k1 : k2;
    // adjacent-unique compaction
    HIPCHK(c, c->ws[WS_MISC0].ensure(std::max<uint64_t>(P, 1)));
    HIPCHK(c, c->ws[WS_MISC1].ensure((P + 2) * 8));
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(std::max<uint64_t>(P, S)) * 8 + 64));
    fd_launch_uniq_flags(keys_s, ids_s, P, c->ws[WS_MISC0].as<uint8_t>(), st);
    fd_exclusive_scan<uint8_t>(c->ws[WS_MISC0].as<uint8_t>(), P, c->ws[WS_MISC1].as<uint64_t>(), c->ws[WS_SCANTMP].as<uint64_t>(),
                               c->ws[WS_TOTAL].as<uint64_t>(), st);
    fd_launch_compact(keys_s, c->ws[WS_MISC0].as<uint8_t>(), c->ws[WS_MISC1].as<uint64_t>(), P, spare, st);
    // hash_off[s] = unique position at the first raw element of structure s (segments survive the stable sort by id)
    HIPCHK(c, c->ws[WS_MISC2].ensure((S + 2) * 8));
    fd_launch_gather_u64(c->ws[WS_MISC1].as<uint64_t>(), c->ws[WS_SEGOFF].as<uint64_t>(), S + 1, c->ws[WS_MISC2].as<uint64_t>(), st);
    HIPCHK(c, hipGetLastError());
    uint64_t U = 0;
    if ((rc = d2h_u64(c, c->ws[WS_TOTAL].as<uint64_t>(), &U))) return rc;
    ib_u32_ptr h((uint32_t *)malloc(std::max<uint64_t>(U, 1) * 4));
    if (!h) return FDGPU_ENOMEM;
    HIPCHK(c, hipMemcpyAsync(h.get(), spare, U * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_off.get(), c->ws[WS_MISC2].p, (S + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *hashes = h.release(); *hash_off = h_off.release();
    return FDGPU_OK;
}

// Raw hash list with positions: every ordered residue pair that has a feature, in the reference's row-major order, as
// (hash, partner residue j); entries [row_off[i], row_off[i + 1]) belong to residue i (batch residue indices).  This is the inner loop of
// collect_hash_id_pos (src/controller/summary.rs:632-690: get_single_feature + perfect_hash for every (i, j)) for a whole batch.
extern "C" int fdgpu_hash_batch_rows(fdgpu_ctx *c, const fdgpu_batch *b, const fd_hash_params *p, uint32_t **hashes, uint32_t **partner, uint64_t **row_off) { FD_LOCK(c);
    if (!c || !b || !p || !hashes || !partner || !row_off) return FDGPU_EINVAL;
    *hashes = nullptr; *partner = nullptr; *row_off = nullptr;
    if (p->n_multiple_bins) FAIL(c, FDGPU_EINVAL, "hash_batch_rows: multiple_bins is honoured by the index build and the query calls only");
    if (!fd_hash_type_supported(p->hash_type)) FAIL(c, FDGPU_EINVAL, "hash_type: unknown encoding");
    reset_timings(c);
    const fd_hash_consts C = make_consts(p);
    const uint64_t R = b->n_res;
    hipStream_t st = c->stream;
    uint64_t P = 0;
    int rc = row_count_and_scan(c, b, C, p->dist_cutoff, &P);
    if (rc) return rc;
    HIPCHK(c, c->ws[WS_KEYS_A].ensure(std::max<uint64_t>(P, 1) * 4));
    HIPCHK(c, c->ws[WS_IDS_A].ensure(std::max<uint64_t>(P, 1) * 4));
    fd_launch_row_emit(b->view(), C, c->ws[WS_MISC1].as<uint64_t>(), c->ws[WS_KEYS_A].as<uint32_t>(), p->dist_cutoff, c->ws[WS_IDS_A].as<uint32_t>(), 0u, st, 1);
    HIPCHK(c, hipGetLastError());
    ib_u32_ptr h((uint32_t *)malloc(std::max<uint64_t>(P, 1) * 4)), pj((uint32_t *)malloc(std::max<uint64_t>(P, 1) * 4));
    ib_u64_ptr ro((uint64_t *)malloc((R + 1) * 8));
    if (!h || !pj || !ro) return FDGPU_ENOMEM;
    hipError_t e = hipMemcpyAsync(h.get(), c->ws[WS_KEYS_A].p, P * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pj.get(), c->ws[WS_IDS_A].p, P * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ro.get(), c->ws[WS_MISC1].p, (R + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { c->err = std::string("hash_batch_rows: ") + hipGetErrorString(e); return FDGPU_EHIP; }
    *hashes = h.release(); *partner = pj.release(); *row_off = ro.release();
    return FDGPU_OK;
}

// ---- S2: the encoder on a sorted stream ------------------------------------------------------------------------------
#define FDGPU_RETRY_WIDE 1000
// WS_MISC3 of a build / encoder call, in u64 words: what the kernels of one call tell the host, and the MSD stream's bucket starts
enum {
    IB_W_TOTALS = 0, IB_W_VALUE_BYTES = 0, IB_W_HASHES = 1, IB_W_POSTINGS = 2,      // the encoder's totals (where its three tile scans end) and the first of them
    IB_W_WIDE = 3,              // a 6-byte form met what it cannot hold: a hash beyond 30 bits (emit), a residue type outside 0..19 (k_frames_perm)
    IB_W_SORT_OVERFLOW = 4,     // the segmented sort met a (bucket, digit) group of 2^32 keys or more
    IB_W_READ = 5,              // words the host reads back behind the sizes pass
    IB_W_BUCKET_STARTS = 8,     // 8-48: the MSD stream's forty bucket starts + its end, written by the sizes pass for the write pass
};
static uint64_t *ib_word(fdgpu_ctx *c, int w) { return c->ws[WS_MISC3].as<uint64_t>() + w; }
static int ib_clear_words(fdgpu_ctx *c) {      // every call's prologue: the slot, and zeros in the words up to the bucket starts
    HIPCHK(c, c->ws[WS_MISC3].ensure(512));
    HIPCHK(c, hipMemsetAsync(c->ws[WS_MISC3].p, 0, IB_W_BUCKET_STARTS * 8, c->stream));
    return FDGPU_OK;
}
// The encoder on a sorted stream of P elements (codec: k_index.hip; S structures; for codec 2 WS_SEGOFF holds the stream's [40][seg_stride] table): sizes
// per tile, their three scans, the totals read back, an index of exactly that size, the write pass.  The caller ran ib_clear_words.  Shared by the
// build and by the fdgpu_debug_encode_stream entries.
static int encode_sorted_stream(fdgpu_ctx *c, const uint32_t *ks, const void *is, int codec, uint64_t first_id, uint64_t P, uint64_t S, uint64_t seg_stride, fdgpu_index **out) {
    hipStream_t st = c->stream;
    const bool el6 = codec != 0;
    const uint32_t nt = std::max<uint32_t>(fd_enc_num_tiles(P), 1);
    for (int s : {WS_TILE_B, WS_TILE_H, WS_TILE_P}) HIPCHK(c, c->ws[s].ensure((size_t)(nt + 1) * 4));
    for (int s : {WS_TILE_BO, WS_TILE_HO, WS_TILE_PO}) HIPCHK(c, c->ws[s].ensure((size_t)(nt + 2) * 8));
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(std::max<uint64_t>(nt, S)) * 8 + 64));
    // per tile: value bytes, hashes and postings it adds, and where each of the three starts (their exclusive scans)
    uint32_t *tile_bytes = c->ws[WS_TILE_B].as<uint32_t>(), *tile_hashes = c->ws[WS_TILE_H].as<uint32_t>(), *tile_posts = c->ws[WS_TILE_P].as<uint32_t>();
    uint64_t *bytes_off = c->ws[WS_TILE_BO].as<uint64_t>(), *hashes_off = c->ws[WS_TILE_HO].as<uint64_t>(), *posts_off = c->ws[WS_TILE_PO].as<uint64_t>();
    uint64_t *scan_tmp = c->ws[WS_SCANTMP].as<uint64_t>();
    const uint64_t *seg = c->ws[WS_SEGOFF].as<uint64_t>();
    uint64_t tot[IB_W_READ] = {0, 0, 0, 0, 0};
    const uint64_t nt_eff = P ? fd_enc_num_tiles(P) : 0;
    {
        StageTimer t(c, "encode_sizes", P * (el6 ? 6 : 8));
        for (uint32_t *tile : {tile_bytes, tile_hashes, tile_posts}) HIPCHK(c, hipMemsetAsync(tile, 0, (size_t)(nt + 1) * 4, st));
        fd_launch_enc_sizes(ks, is, codec, (uint32_t)first_id, P, tile_bytes, tile_hashes, tile_posts, seg, seg_stride, ib_word(c, IB_W_BUCKET_STARTS), st);
        fd_exclusive_scan<uint32_t>(tile_bytes, nt_eff, bytes_off, scan_tmp, ib_word(c, IB_W_VALUE_BYTES), st);
        fd_exclusive_scan<uint32_t>(tile_hashes, nt_eff, hashes_off, scan_tmp, ib_word(c, IB_W_HASHES), st);
        fd_exclusive_scan<uint32_t>(tile_posts, nt_eff, posts_off, scan_tmp, ib_word(c, IB_W_POSTINGS), st);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(tot, ib_word(c, IB_W_TOTALS), sizeof tot, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (tot[IB_W_SORT_OVERFLOW]) FAIL(c, FDGPU_ERANGE, "index build: one (residue-pair bucket, key digit) group holds 2^32 keys or more; build the shard in several calls and merge");
    if (el6 && tot[IB_W_WIDE]) return FDGPU_RETRY_WIDE;
    fdgpu_index *ix = nullptr;
    const int rc = fd_index_new(c, true, tot[IB_W_HASHES], tot[IB_W_VALUE_BYTES], true, &ix);
    if (rc) return rc;
    ix->n_postings = tot[IB_W_POSTINGS]; ix->n_structures = S; ix->first_id = first_id;
    {
        StageTimer t(c, "encode_write", P * (el6 ? 6 : 8) + ix->value_len + ix->n_hashes * 12);
        fd_launch_enc_write(ks, is, codec, (uint32_t)first_id, P, bytes_off, hashes_off, ix->value, ix->hashes, ix->offsets, ix->last_ids, ib_word(c, IB_W_TOTALS), ix->n_hashes,
                            ib_word(c, IB_W_BUCKET_STARTS), st);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { c->err = std::string("encode launch: ") + hipGetErrorString(e); fdgpu_index_destroy(ix); return FDGPU_EHIP; }
    *out = ix;
    return FDGPU_OK;
}

// ---- S2: the build = choose form -> count -> limits -> emit -> sort -> encode ------------------------------------------------
// The three builds.  OWN: the encodings with their own descriptor go one ordered pair at a time through the row kernels (reference order), 8-byte
// elements.  STRUCTURE_MAJOR: keys in structure order, four 8-bit sort passes; shards of <= 2^18 structures use 6-byte elements (key = hash << 2 |
// local id bits 17:16, u16 payload) as long as every hash fits 30 bits, the 8-byte form (u32 hash, u32 id) otherwise; --multiple-bins is built here.
// MSD (default encoding, 6-byte elements): the pair kernel writes the keys partitioned by the top six hash bits (forty buckets, residues visited in
// amino-acid order) and every bucket is sorted by the remaining 24 bits — three passes instead of four; the bucket carries the top six hash bits:
// u32 plane = hash[7:0] << 24 | local id, u16 plane = hash[23:8] — 2^24 structures.  FDGPU_MSD=0 selects the structure-major build (A/B measurements, tests).
enum ib_kind { IB_OWN, IB_STRUCTURE_MAJOR, IB_MSD };
static const uint32_t IB_BUCKETS = 40;
struct ib_form {
    ib_kind kind; bool el6; int codec;      // el6: 6-byte sort elements (a u32 and a u16 plane), else 8-byte; codec: of the sorted stream (k_index.hip)
    uint32_t n_cfg; uint64_t seg_stride;      // bin pairs of --multiple-bins (1 without); the encoder's entries per bucket of the [bucket][work item] table (0 without)
    uint64_t max_keys; const char *too_many;      // keys are addressed with 32 bits; by MSD with 64 (one call then covers 2^18 AFDB-shaped structures: ~8.7e9 keys, 105 GB to sort)
};
// The form, and the refusals of a build's arguments.  force32: 8-byte sort elements (FDGPU_IDS32, or the retry).
static int ib_choose_form(fdgpu_ctx *c, const fdgpu_batch *b, const fd_hash_params *p, uint64_t first_id, bool force32, ib_form &F) {
    if (!fd_hash_type_supported(p->hash_type)) FAIL(c, FDGPU_EINVAL, "hash_type: only the encodings over the (d_CA, d_CB, theta, tau1, tau2) descriptor are built (0, 1, 3, 7, 8)");
    reset_timings(c);      // (behind the first refusal: a call refused for its encoding leaves the previous call's timings)
    const uint64_t S = b->n_struct;
    if (first_id + S > 0xffffffffull) FAIL(c, FDGPU_ERANGE, "structure ids exceed 32 bits");
    if (!fd_multiple_bins_valid(p)) FAIL(c, FDGPU_EINVAL, "multiple_bins: at most 8 (dist, angle) bin pairs, no zero counts");
    F.n_cfg = fd_num_bin_configs(p);
    const bool own = fd_own_descriptor(p->hash_type);
    if (own && F.n_cfg > 1) FAIL(c, FDGPU_EINVAL, "multiple_bins is built for the encodings over the PDBTrRosetta descriptor only");
    const bool ids16 = !own && !force32 && S <= (1ull << 18);
    const bool msd_env = [] { const char *e = getenv("FDGPU_MSD"); return !(e && e[0] == '0'); }();      // read per call: tests flip it
    const bool msd = msd_env && !own && !force32 && S <= (1ull << 24) && F.n_cfg == 1 && p->hash_type == FDGPU_HASH_PDBTR && S > 0;
    F.kind = own ? IB_OWN : msd ? IB_MSD : IB_STRUCTURE_MAJOR;
    F.el6 = ids16 || msd;
    F.codec = msd ? 2 : ids16 ? 1 : 0;
    F.seg_stride = msd ? b->n_work : 0;
    F.max_keys = msd ? 1ull << 35 : 0xffffffffull;
    F.too_many = msd ? "more than 2^35 residue pairs in one build call; split the shard" : "more than 2^32 residue pairs in one build call; split the shard";
    return FDGPU_OK;
}
// frames of every residue in batch order (own, structure-major)
static void ib_frames(fdgpu_ctx *c, const fdgpu_batch *b) {
    StageTimer t(c, "frames", b->n_res * (37 + sizeof(fd_frame)));
    fd_launch_frames(b->view(), b->n_res, c->ws[WS_FRAMES].p, c->stream);
}
// MSD count: the residues in amino-acid order (V: the view of that order, which the emit takes too), then counts[bucket][work item] (the count pass
// writes every entry: nothing to clear, and it makes the frames of its tile) and their exclusive scan in WS_SEGOFF, which IS the bucket-major layout —
// every work item's slots in it are its own.  -> FDGPU_RETRY_WIDE when k_frames_perm met a residue type outside 0..19: no point in finishing this form.
// PAIR MASKS: the count pass also stores the pass mask of every (work item, partner) — one u64 per column of b->wi_col, WS_PAIR_MASKS — and the emit
// pass replays them instead of running the distance filter a second time (k_hash.hip: fd_replay_block).  The table is a convenience, never a
// condition: without it (FDGPU_PAIR_MASKS=0, read per call; a pair kernel other than the default one; a device that cannot hold it) the count pass
// stores nothing and the emit pass filters, as both always did.  *masks: the table, or null.
static bool ib_pair_masks_wanted(const fdgpu_ctx *c, const fd_hash_consts &C) {
    const char *e = getenv("FDGPU_PAIR_MASKS");
    return !(e && e[0] == '0') && C.use_tab == 3 && !c->pair_masks_crowded;
}
static int ib_count_msd(fdgpu_ctx *c, const fdgpu_batch *b, const fd_hash_consts &C, fd_batch_view &V, uint64_t *P1, uint64_t **masks) {
    hipStream_t st = c->stream;
    const uint64_t R1 = std::max<uint64_t>(b->n_res, 1), NS = (uint64_t)IB_BUCKETS * b->n_work;
    HIPCHK(c, c->ws[WS_CA_PERM].ensure(R1 * 12));
    HIPCHK(c, c->ws[WS_OK_PERM].ensure(R1));
    HIPCHK(c, c->ws[WS_AA_PERM].ensure(R1));
    HIPCHK(c, c->ws[WS_SRC_PERM].ensure(R1 * 4));
    V = b->view();
    {
        StageTimer t(c, "frames", b->n_res * (2 + 14 + 18));      // the permutation alone: types and flags for the totals, then 14 B read and 18 B written per residue
        fd_launch_frames_perm(V, c->ws[WS_CA_PERM].as<float>(), c->ws[WS_OK_PERM].as<uint8_t>(), c->ws[WS_AA_PERM].as<uint8_t>(), c->ws[WS_SRC_PERM].as<uint32_t>(),
                              C.wide_flag, st);
    }
    V.ca_xyz = c->ws[WS_CA_PERM].as<float>(); V.hash_ok = c->ws[WS_OK_PERM].as<uint8_t>(); V.aa = c->ws[WS_AA_PERM].as<uint8_t>();
    V.n_xyz = nullptr; V.cb_xyz = nullptr;      // the emit reads frames, not atoms; the count pass, which builds the frames, gets the batch's N / CB beside the view
    HIPCHK(c, c->ws[WS_COUNTS].ensure((NS + 1) * 4));
    HIPCHK(c, c->ws[WS_SEGOFF].ensure((NS + 2) * 8));
    HIPCHK(c, c->ws[WS_SCANTMP].ensure(fd_scan_tmp_elems(std::max<uint64_t>(NS, b->n_res)) * 8 + 64));
    HIPCHK(c, c->ws[WS_TOTAL].ensure(64));
    *masks = nullptr;
    if (ib_pair_masks_wanted(c, C) && b->wi_col) {
        if (c->ws[WS_PAIR_MASKS].ensure((b->n_mask_cols + FD_MASK_SLACK_WORDS) * 8) == hipSuccess) *masks = c->ws[WS_PAIR_MASKS].as<uint64_t>();
        else (void)hipGetLastError();      // no room for it: this call filters twice
    }
    {
        // per residue: CA, flag and type of the filter (14 B), the source index, N and CB (28 B) and the frame it stores; + the table.  The mask
        // table's bytes (written here, read by the emit) are NOT in the stages' figures: tests/test_gpu_build_stage_lists.py pins those; they are
        // reported on their own (fdgpu_debug_last_build_mask_bytes)
        StageTimer t(c, "pair_count", b->n_res * (14 + 28 + sizeof(fd_frame)) + NS * 4);
        fd_launch_pair_count_msd(V, C, b->n_xyz, b->cb_xyz, c->ws[WS_SRC_PERM].as<uint32_t>(), c->ws[WS_FRAMES].p, c->ws[WS_COUNTS].as<uint32_t>(), *masks, st);
    }
    int rc = scan_counts(c, NS, P1);
    uint64_t odd = 0;
    if (!rc) rc = d2h_u64(c, (const uint64_t *)C.wide_flag, &odd);
    return !rc && odd ? FDGPU_RETRY_WIDE : rc;
}
static int ib_reserve_keys(fdgpu_ctx *c, const ib_form &F, uint64_t P, ib_keys &K) { return reserve_keys(c, P, F.max_keys, F.too_many, F.el6 ? 2 : 4, K); }
static void ib_emit_rows(fdgpu_ctx *c, const fdgpu_batch *b, const fd_hash_params *p, const fd_hash_consts &C, const ib_keys &K, uint64_t P, uint64_t first_id) {
    StageTimer t(c, "pair_emit", b->n_res * 37 + P * 8);
    fd_launch_row_emit(b->view(), C, c->ws[WS_MISC1].as<uint64_t>(), K.ka, p->dist_cutoff, (uint32_t *)K.ia, (uint32_t)first_id, c->stream);
}
static void ib_emit_msd(fdgpu_ctx *c, const fdgpu_batch *b, const fd_batch_view &V, const fd_hash_consts &C, const ib_keys &K, uint64_t P, const uint64_t *masks) {
    StageTimer t(c, "pair_emit", b->n_res * 37 + P * 6);
    c->last_build_mask_bytes = masks ? b->n_mask_cols * 8 : 0;
    fd_launch_pair_emit_msd(V, c->ws[WS_FRAMES].p, C, c->ws[WS_SEGOFF].as<uint64_t>(), K.ka, (uint16_t *)K.ia, masks, c->stream);
}
// every bin pair of --multiple-bins contributes one key per ordered residue pair: one emit per pair, each from a cleared cursor
static int ib_emit_structure_major(fdgpu_ctx *c, const fdgpu_batch *b, const fd_hash_params *p, const ib_form &F, const fd_hash_consts &C, const ib_keys &K, uint64_t P,
                                   uint64_t first_id) {
    StageTimer t(c, "pair_emit", b->n_res * 37 + P * (F.el6 ? 6 : 8));
    for (uint32_t k = 0; k < F.n_cfg; ++k) {
        fd_hash_consts Ck = fd_make_consts_cfg(p, k);
        Ck.spec_miss = C.spec_miss; Ck.wide_flag = C.wide_flag; Ck.seg_mul = F.n_cfg; Ck.seg_cfg = k;
        if (k) HIPCHK(c, hipMemsetAsync(c->ws[WS_CURSOR].p, 0, (b->n_struct + 1) * 4, c->stream));
        fd_launch_pair_emit2(b->view(), c->ws[WS_FRAMES].p, Ck, c->ws[WS_SEGOFF].as<uint64_t>(), c->ws[WS_CURSOR].as<uint32_t>(), K.ka, K.ia, F.el6, (uint32_t)first_id,
                             c->stream);
    }
    return FDGPU_OK;
}
// the sorts return which buffer pair holds the result (0: a, 1: b)
static int ib_sort(fdgpu_ctx *c, const ib_form &F, const ib_keys &K, uint64_t P) {      // own, structure-major: all 32 key bits (unmasked field overflow can set bits 30-31)
    if (F.el6) return fd_radix_sort_pairs16(K.ka, (uint16_t *)K.ia, K.kb, (uint16_t *)K.ib, P, 32, c->ws[WS_GHIST].as<uint32_t>(), c->ws[WS_TOT].as<uint64_t>(), c->stream, c);
    return sort_pairs(c, K.ka, (uint32_t *)K.ia, K.kb, (uint32_t *)K.ib, P, 32);
}
// MSD: every bucket by hash bits [0, 24): three passes (hash[7:0] = u32 plane bits 31:24, hash[23:8] = the u16 plane); the bucket holds the other six
static int ib_sort_msd(fdgpu_ctx *c, const fdgpu_batch *b, const ib_keys &K, uint64_t P, int *cur) {
    static const fd_rs_digit digits[3] = {{0, 24}, {1, 0}, {1, 8}};
    HIPCHK(c, c->ws[WS_GHIST].ensure((size_t)256 * fd_rs_seg_num_tiles(P, IB_BUCKETS) * 4));
    HIPCHK(c, c->ws[WS_TOT].ensure(fd_rs_seg_tot_words(P, IB_BUCKETS) * 8));
    HIPCHK(c, c->ws[WS_SEG_TAB].ensure(fd_rs_seg_tab_bytes(P, IB_BUCKETS)));
    *cur = fd_radix_sort_pairs16_seg(K.ka, (uint16_t *)K.ia, K.kb, (uint16_t *)K.ib, P, c->ws[WS_SEGOFF].as<uint64_t>(), b->n_work, IB_BUCKETS, digits, 3,
                                     c->ws[WS_GHIST].as<uint32_t>(), c->ws[WS_TOT].as<uint64_t>(), c->ws[WS_SEG_TAB].p, c->stream, c,
                                     (unsigned long long *)ib_word(c, IB_W_SORT_OVERFLOW));
    return FDGPU_OK;
}

// Returns FDGPU_RETRY_WIDE (internal) when a 6-byte form met a hash beyond 30 bits or a residue type outside 0..19.
static int index_build_impl(fdgpu_ctx *c, const fdgpu_batch *b, const fd_hash_params *p, uint64_t first_id, fdgpu_index **out, bool force32) {
    if (!c || !b || !p || !out) return FDGPU_EINVAL;
    *out = nullptr;
    ib_form F;
    int rc = ib_choose_form(c, b, p, first_id, force32, F);
    if (rc) return rc;
    c->last_build_mask_bytes = 0;
    HIPCHK(c, c->ws[WS_FRAMES].ensure(std::max<uint64_t>(b->n_res, 1) * sizeof(fd_frame)));
    if ((rc = ib_clear_words(c))) return rc;
    fd_hash_consts C = fd_make_consts_cfg(p, 0);
    C.spec_miss = c->spec_miss;
    C.wide_flag = (unsigned long long *)ib_word(c, IB_W_WIDE);
    uint64_t P = 0;
    ib_keys K;
    fd_batch_view V;
    int cur = 0;
    switch (F.kind) {      // the one place that tells the forms apart: each is its sequence of stages
    case IB_OWN:
        ib_frames(c, b);
        if ((rc = row_count_and_scan(c, b, C, p->dist_cutoff, &P, "pair_count")) || (rc = ib_reserve_keys(c, F, P, K))) return rc;
        ib_emit_rows(c, b, p, C, K, P, first_id);
        cur = ib_sort(c, F, K, P);
        break;
    case IB_STRUCTURE_MAJOR:
        ib_frames(c, b);
        if ((rc = count_and_scan(c, b, C, &P, true))) return rc;
        P *= F.n_cfg;
        if ((rc = ib_reserve_keys(c, F, P, K)) || (rc = ib_emit_structure_major(c, b, p, F, C, K, P, first_id))) return rc;
        cur = ib_sort(c, F, K, P);
        break;
    case IB_MSD: {
        uint64_t *masks = nullptr;
        if ((rc = ib_count_msd(c, b, C, V, &P, &masks)) || (rc = ib_reserve_keys(c, F, P, K))) return rc;
        ib_emit_msd(c, b, V, C, K, P, masks);
        if ((rc = ib_sort_msd(c, b, K, P, &cur))) return rc;
        break;
    }
    }
    return encode_sorted_stream(c, cur ? K.kb : K.ka, cur ? K.ib : K.ia, F.codec, first_id, P, b->n_struct, F.seg_stride, out);
}

extern "C" int fdgpu_index_build(fdgpu_ctx *c, const fdgpu_batch *b, const fd_hash_params *p, uint64_t first_id, fdgpu_index **out) { FD_LOCK(c);
    const char *e32 = getenv("FDGPU_IDS32");   // FDGPU_IDS32=1 forces the 8-byte sort elements (read per call: tests flip it)
    int rc = index_build_impl(c, b, p, first_id, out, e32 && e32[0] == '1');
    if (rc == FDGPU_RETRY_WIDE) rc = index_build_impl(c, b, p, first_id, out, true);
    if (rc == FDGPU_EHIP && c && c->ws[WS_PAIR_MASKS].p) {
        // a HIP call failed with the mask table on the device — the sort buffers or the index may not fit beside it: the table goes back, this
        // call is made again without it and so are the following ones (until fdgpu_release_workspaces)
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        c->ws[WS_PAIR_MASKS].release();
        c->pair_masks_crowded = true;
        rc = index_build_impl(c, b, p, first_id, out, e32 && e32[0] == '1');
        if (rc == FDGPU_RETRY_WIDE) rc = index_build_impl(c, b, p, first_id, out, true);
    }
    return rc;
}

extern "C" int fdgpu_debug_last_build_mask_bytes(fdgpu_ctx *c, uint64_t *bytes) { FD_LOCK(c);
    if (!c || !bytes) return FDGPU_EINVAL;
    *bytes = c->last_build_mask_bytes;
    return FDGPU_OK;
}

// ---- test-only (include/fdgpu_debug.h) ---------------------------------------------------------------------------------
// the entries' prologue: timings reset, words cleared, the caller's two planes (id_bytes per payload) in WS_KEYS_A / WS_IDS_A
static int debug_upload_stream(fdgpu_ctx *c, const uint32_t *keys, const void *ids, size_t id_bytes, uint64_t n) {
    reset_timings(c);
    const int rc = ib_clear_words(c);
    if (rc) return rc;
    HIPCHK(c, c->ws[WS_KEYS_A].ensure(std::max<uint64_t>(n, 1) * 4));
    HIPCHK(c, c->ws[WS_IDS_A].ensure(std::max<uint64_t>(n, 1) * id_bytes));
    if (n) {
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_KEYS_A].p, keys, n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->ws[WS_IDS_A].p, ids, n * id_bytes, hipMemcpyHostToDevice, c->stream));
    }
    return FDGPU_OK;
}
// The encoder alone on a caller-made stream, 8-byte elements (codec 0).
extern "C" int fdgpu_debug_encode_stream(fdgpu_ctx *c, const uint32_t *hashes, const uint32_t *ids, uint64_t n, fdgpu_index **out) { FD_LOCK(c);
    if (!c || !out || (n && (!hashes || !ids))) return FDGPU_EINVAL;
    *out = nullptr;
    if (n >= 0xffffffffull) FAIL(c, FDGPU_ERANGE, "encode_stream: 2^32 elements or more");
    uint64_t S = 0;
    for (uint64_t p = 0; p < n; ++p) {
        if (p && (hashes[p - 1] > hashes[p] || (hashes[p - 1] == hashes[p] && ids[p - 1] > ids[p]))) FAIL(c, FDGPU_EINVAL, "encode_stream: the stream is not sorted by (hash, id)");
        S = std::max<uint64_t>(S, (uint64_t)ids[p] + 1);
    }
    const int rc = debug_upload_stream(c, hashes, ids, 4, n);
    if (rc) return rc;
    return encode_sorted_stream(c, c->ws[WS_KEYS_A].as<uint32_t>(), c->ws[WS_IDS_A].p, 0, 0, n, S, 0, out);
}
// The same on the 6-byte elements of the MSD build's stream (codec 2), packed here on the host; the 41 bucket starts go to WS_SEGOFF at stride 1.
// The stream is checked before the context is looked at: without one (ctx NULL) the call is those checks alone, which a test without a device can reach.
extern "C" int fdgpu_debug_encode_stream_b24(fdgpu_ctx *c, const uint32_t *hashes, const uint32_t *local_ids, uint64_t n, uint64_t first_id, fdgpu_index **out) { FD_LOCK(c);
    if (!out || (n && (!hashes || !local_ids))) return FDGPU_EINVAL;
    *out = nullptr;
    const uint32_t NB = IB_BUCKETS;
    uint64_t S = 0;
    const char *why = n >= 0xffffffffull ? "encode_stream_b24: 2^32 elements or more" : nullptr;
    for (uint64_t p = 0; p < n && !why; ++p) {
        const uint32_t h = hashes[p], id = local_ids[p];
        if (h >= (1u << 30) || (h >> 24) >= NB) why = "encode_stream_b24: a hash of 2^30 or more, or in a bucket (hash >> 24) of 40 or more";
        else if (id >= (1u << 24)) why = "encode_stream_b24: a local id of 2^24 or more";
        else if (p && (hashes[p - 1] > h || (hashes[p - 1] == h && local_ids[p - 1] > id))) why = "encode_stream_b24: the stream is not sorted by (hash, id)";
        S = std::max<uint64_t>(S, (uint64_t)id + 1);
    }
    if (!why && first_id + S > 0xffffffffull) why = "encode_stream_b24: structure ids exceed 32 bits";
    if (why) { if (c) c->err = why; return FDGPU_EINVAL; }
    if (!c) return FDGPU_OK;
    std::vector<uint32_t> k32(std::max<uint64_t>(n, 1));
    std::vector<uint16_t> v16(std::max<uint64_t>(n, 1));
    std::vector<uint64_t> seg(NB + 2, 0);      // seg[b + 1] counts bucket b, then the running sum: seg[b] = where bucket b starts, seg[40] = n
    for (uint64_t p = 0; p < n; ++p) {
        const uint32_t h = hashes[p];
        k32[p] = (h & 0xffu) << 24 | local_ids[p];
        v16[p] = (uint16_t)(h >> 8);
        ++seg[(h >> 24) + 1];
    }
    for (uint32_t b = 0; b < NB; ++b) seg[b + 1] += seg[b];
    const int rc = debug_upload_stream(c, k32.data(), v16.data(), 2, n);
    if (rc) return rc;
    HIPCHK(c, c->ws[WS_SEGOFF].ensure((NB + 2) * 8));
    HIPCHK(c, hipMemcpyAsync(c->ws[WS_SEGOFF].p, seg.data(), (NB + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the host vectors go out of scope with this call
    return encode_sorted_stream(c, c->ws[WS_KEYS_A].as<uint32_t>(), c->ws[WS_IDS_A].p, 2, first_id, n, S, 1, out);
}
