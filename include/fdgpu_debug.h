/* fdgpu_debug.h — test-only entry points of libfdgpu.so.  Not part of the drop-in boundary (include/fdgpu.h): a host binding does not need
 * them; the parity tests do (tests/ include both).  Same conventions: error codes, library-allocated outputs released by fdgpu_free. */
#ifndef FDGPU_DEBUG_H
#define FDGPU_DEBUG_H
#include "fdgpu.h"
#ifdef __cplusplus
extern "C" {
#endif

/* What every rank runs after the all-gather of fdgpu_sharded_count_query_maps — unpack, global selection, ranking, all on the device — on `world`
 * messages (format: fdgpu_comm_message_bytes in fdgpu.h) given as one host array: tests drive the multi-rank code with it on a single GPU.
 * 0 < top_n <= 3072. */
int fdgpu_debug_merge_gathered(fdgpu_ctx *ctx, uint32_t world, uint64_t n_queries, uint32_t top_n, const uint8_t *messages,
                               fd_count_rec **out, uint64_t **out_off);
/* The unpack + merge step of fdgpu_sharded_retrieve alone, on hand-made contributions of `world` ranks (host arrays): counts[r * (n_queries + 1) + t]
 * = matches rank r found for query t, counts[r * (n_queries + 1) + n_queries] = its status (0 = fine); rank_matches[r] / rank_residues[r] = its
 * records (cand = slot in the query's GLOBAL candidate list) and residue ints in (query, slot, component) order; nres_per[t] = residue ints per
 * match of query t (2 * n_indices).  Output as fdgpu_retrieve_batch.  Lets a single-GPU test drive the multi-rank merge with ragged, empty and
 * failing ranks. */
int fdgpu_debug_merge_retrieved(fdgpu_ctx *ctx, uint32_t world, uint64_t n_queries, const uint64_t *counts, const fd_match_rec *const *rank_matches,
                                const int32_t *const *rank_residues, const uint64_t *nres_per, fd_match_rec **matches, uint64_t **match_off,
                                int32_t **residues, uint64_t **res_off);
/* The ingest's own gzip decoder (csrc/fd_inflate.cpp; the reference reads .gz through the flate2 crate, src/structure/io/pdb.rs:79-124) on a
 * buffer: every member of in[0 .. n) concatenated into *out (fdgpu_free).  FDGPU_EINVAL = the decoder declines the input (damaged, or a code it
 * does not handle); fdgpu_parse_structures then reads that file through zlib.  FDGPU_ZLIB=1 in the environment sends every file there. */
int fdgpu_debug_gunzip(const uint8_t *in, uint64_t n, uint8_t **out, uint64_t *n_out);
/* Evaluates the device restatements of glibc's sinf / cosf / acosf / atanf / atan2f (csrc/fd_libm.h) on arrays, so that tests can compare the
 * gfx950 arithmetic bit for bit with the host.  op: 0 sinf, 1 cosf, 2 acosf, 3 atanf, 4 atan2f(a, b). */
int fdgpu_debug_libm(fdgpu_ctx *ctx, int op, const float *a, const float *b, float *out, uint64_t n);

/* The posting encoder alone (csrc/k_index.hip: the sizes pass, the scans, the write pass — the tail of fdgpu_index_build) on a stream the caller
 * made: n elements (hashes[p], ids[p]) sorted by (hash, id), equal neighbours allowed (they collapse to one posting), as the 8-byte elements of
 * the build (u32 hash, u32 id; first_id 0).  *out: a resident index of max(ids) + 1 structures, released with fdgpu_index_destroy.  Lets a test
 * place list heads, varint lengths, duplicates and byte alignments where proteins never put them.  FDGPU_EINVAL for an unsorted stream. */
int fdgpu_debug_encode_stream(fdgpu_ctx *ctx, const uint32_t *hashes, const uint32_t *ids, uint64_t n, fdgpu_index **out);
/* The same on the 6-byte elements of the default build's stream (codec 2 of csrc/k_index.hip), which the entry above does not reach: the stream
 * (hashes[p], first_id + local_ids[p]), sorted by (hash, local id), is packed on the host into the two planes (u32 = hash[7:0] << 24 | local id,
 * u16 = hash[23:8]) and the 41 starts of the buckets hash >> 24.  Requires hash < 2^30, hash >> 24 < 40 and local id < 2^24; FDGPU_EINVAL for
 * anything else and for an unsorted stream.  *out: a resident index of max(local_ids) + 1 structures with that first_id.  The stream is checked
 * before the context is used: with ctx NULL the call is the checks alone (FDGPU_OK for a stream it would encode, *out stays NULL), which a test
 * without a device can reach. */
int fdgpu_debug_encode_stream_b24(fdgpu_ctx *ctx, const uint32_t *hashes, const uint32_t *local_ids, uint64_t n, uint64_t first_id, fdgpu_index **out);

/* Host-only pieces of the retrieval glue for graphs of more than 64 nodes (csrc/fd_host_query.hip), callable without a GPU.
 * fdgpu_debug_host_components: the graph of the found residue pairs (edge_i[e] -> edge_j[e], nodes numbered by first appearance,
 * src/controller/graph.rs:16-26) and its strongly + weakly connected components of at least node_count nodes, each sorted by node, the list sorted
 * and without duplicates (graph.rs:29-50).  Component k holds (*residues)[(*comp_off)[k] .. (*comp_off)[k + 1]) — the RESIDUES of its nodes in node
 * order; both arrays are released with libc free().
 * fdgpu_debug_hash_is_symmetric: out[k] = the symmetry flag of hashes[k] for the encoding (geometry/pdb_tr.rs:158-162 and the other encodings'
 * is_symmetric). */
int fdgpu_debug_host_components(const uint32_t *edge_i, const uint32_t *edge_j, uint64_t n_edges, uint32_t node_count, uint32_t **residues,
                                uint64_t **comp_off, uint64_t *n_comps);
int fdgpu_debug_hash_is_symmetric(uint32_t hash_type, const uint32_t *hashes, uint64_t n, uint8_t *out);
/* fdgpu_debug_host_retrieve_slot: what the host path of fdgpu_retrieve_batch computes on its threads for ONE candidate slot (csrc/fd_retrieve_host.cpp:
 * graph -> components -> votes -> assignment -> rescue -> residue lists), from a pair scan's output given as arrays: the slot's found triples
 * (found_i, found_j, found_hash)[n_found] in scan order (residues below n_target, else FDGPU_EINVAL) and its candidate pairs (cand_qi, cand_i,
 * cand_j)[n_pairs] (out-of-range fields are ignored like the glue ignores them), the target's residue count, the query map, hash_type, node_count.
 * two_pass != 0: the two-scan form of large queries — the plan pass on the found triples alone, then only the candidate pairs the second scan
 * returns (partner residue cand_j marked by the plan pass), then the full pass on the cached plans.  packed != 0: the candidate pairs reach the slot
 * in the scan's packed form (16 bits a field: FDGPU_EINVAL beyond), else as records.  Out: *n_recs records in emission order (component order,
 * graph.rs:43-45): (*idf)[k], (*same)[k], and (*residues)[k * 2 * n_indices ...] = the from-hash list then the processed list (-1 = none).  No
 * coordinates, no superposition.  The three arrays are released with libc free(). */
int fdgpu_debug_host_retrieve_slot(const uint32_t *found_i, const uint32_t *found_j, const uint32_t *found_hash, uint64_t n_found, const uint32_t *cand_qi,
                                   const uint32_t *cand_i, const uint32_t *cand_j, uint64_t n_pairs, uint32_t n_target, const fd_query_map *qm,
                                   uint32_t hash_type, uint32_t node_count, uint32_t two_pass, uint32_t packed, uint64_t *n_recs, float **idf,
                                   uint32_t **same, int32_t **residues);

/* The host block a pair scan (fdgpu_match_pairs and the retrieval's scans) sends to the device before its first launch (csrc/fd_match_tables.cpp), built
 * without a device: query t scans the structures cand[cand_off[t] .. cand_off[t + 1]) of a batch of n_struct structures whose residues start at
 * res_off[0 .. n_struct] (only lengths are read).  dev_items != 0: the form whose work items the device writes (every candidate's first item and query),
 * else the four host-built item arrays.  pooled != 0: interval tables of queries with 8,192 observed distances and more on helper threads.
 * Out: *block = the packed block (padding zeroed; libc free()), layout[16] = the word offsets of its sections {cand, wc, wi, wq, wj, hashes, start,
 * dist, qi, qtab, iv_start, iv, iv_grp, wbase, cq} and its length in words, scalars[5] = {work items, j_span, interval tables built, hash-set slots,
 * largest hash count of a query with a set}.  On FDGPU_EINVAL / FDGPU_ERANGE *message is the text the scan would leave as the context's error. */
int fdgpu_debug_match_tables(uint64_t n_queries, const fd_match_query *qs, const uint32_t *cand, const uint64_t *cand_off, const uint64_t *res_off,
                             uint64_t n_struct, uint32_t hash_type, uint32_t dev_items, uint32_t pooled, uint32_t **block, uint64_t *layout,
                             uint64_t *scalars, const char **message);

/* Which form the LAST count call on this context took (fdgpu_count_query, fdgpu_count_query_batch[_top], fdgpu_count_query_maps_top): the
 * booleans its dispatch computed, one bit each, so that a test at one of the dispatch's switches can tell which side it landed on.
 * OVERFLOW: the device selection met more ties at a cut than it holds and the call was ranked again by the compacting path — the other bits then
 * still describe the first attempt.  0 = no count call yet, or one that returned before the dispatch (no structures, no rows). */
#define FDGPU_PATH_TILED 1u          /* scores per tile of structures in LDS (k_qtile.hip / k_qscore32.hip) */
#define FDGPU_PATH_SUMS32 2u         /* 32-bit idf sums over the planned slot stream (k_qscore32.hip) */
#define FDGPU_PATH_STREAM 4u         /* pass B reads the decoded stream pass A left */
#define FDGPU_PATH_SLICED 8u         /* one query of thousands of rows on the tiles, rows in slices */
#define FDGPU_PATH_ROWS 16u          /* occupancy rows (k_query.hip) */
#define FDGPU_PATH_PACKED 32u        /* packed (count, idf sum) accumulators: every row's idf below 32 */
#define FDGPU_PATH_OVERFLOW 64u      /* selection overflow, ranked by the compacting path */
int fdgpu_debug_last_count_path(fdgpu_ctx *ctx, uint32_t *flags);

/* The LAST fdgpu_index_build call on this context: the bytes of the mask table its emit pass replayed (8 per column: one u64 per work item and
 * partner, work items padded to blocks of 64 partners; written once by the count pass, read once), or 0 when the emit pass ran the distance filter
 * itself (FDGPU_PAIR_MASKS=0, a build form or pair kernel without the table, no room on the device).  These bytes are not part of the stages'
 * byte figures (fdgpu_last_timings). */
int fdgpu_debug_last_build_mask_bytes(fdgpu_ctx *ctx, uint64_t *bytes);

/* Which way the LAST fdgpu_retrieve / fdgpu_retrieve_batch call on this context went (tests at the dispatch's switches): stage names alone cannot
 * tell a call that the device glue declined from one that never started it.  0 = no such call yet. */
#define FDGPU_RPATH_DEVICE_TRIED 1u  /* the device glue (k_retrieve.hip) was started */
#define FDGPU_RPATH_DEVICE_DONE 2u   /* ... and produced the result */
#define FDGPU_RPATH_LIMIT 4u         /* ... a slot beyond the kernel's limits (nodes, found triples, lists): host path for the whole call */
#define FDGPU_RPATH_CAPACITY 8u      /* ... the output buffers' capacity: host path for the whole call */
#define FDGPU_RPATH_TWO_PASS 16u     /* found triples and candidate pairs in two scans */
#define FDGPU_RPATH_SPLIT 32u        /* the device glue in its split form (k_rs_setup / k_rs_comp, k_rs_slots for the listed slots) */
int fdgpu_debug_last_retrieve_path(fdgpu_ctx *ctx, uint32_t *flags);

/* Which form the LAST fdgpu_make_query_map[_batch] call on this context took for "candidates -> hashes" (csrc/fd_query_map.hip, qm_choose_form: the
 * only place that sets them).  A call refused before the form is chosen (bad arguments, hash type, multiple_bins) leaves the previous call's flags. */
#define FDGPU_QMPATH_HOST_EXPAND 1u      /* candidates expanded on the host, their containers hashed per bin configuration */
#define FDGPU_QMPATH_DEVICE_EXPAND 2u    /* expanded and hashed on the device (k_qm_expand_hash); alone: hashes only, first insertions and lengths on the host */
#define FDGPU_QMPATH_CHAIN 4u            /* ... then first insertions per query in LDS (k_qm_dedupe) */
#define FDGPU_QMPATH_CHAIN_LENGTHS 8u    /* ... and every candidate's posting length in the same chain (an index was given) */
#define FDGPU_QMPATH_SORT_DEDUPE 16u     /* ... or, one large query: first insertions by a device sort */
int fdgpu_debug_last_query_map_path(fdgpu_ctx *ctx, uint32_t *flags);

/* The host steps of make_query_map (csrc/fd_query_map_host.cpp), callable without a context or a device.  Output arrays are released with libc free().
 * fdgpu_debug_qm_pairs: the ordered residue pairs of queries (q_struct, q_off, q_index as fdgpu_make_query_map_batch) over a batch whose residues
 *   start at res_off[]: *pair_i / *pair_j hold batch-wide residue indices, query t's pairs are [pair_off[t], pair_off[t + 1]) (pair_off: n_queries + 1).
 * fdgpu_debug_qm_fields: out[12] = {n_dist_fields, dist_field[2], n_angle_fields, angle_field[7], takes substitutions}, unused entries -1.
 * fdgpu_debug_qm_expand: the host expansion of ONE query's pairs (features[n_pairs][12], valid[n_pairs]; the query's structure starts at residue r0;
 *   subs / n_subs parallel to q_index[n_q], or NULL; angle thresholds in RADIANS): *cand_features = [n][12], *cand_recs = [n][4] = (qi, qj, observed?, pair).
 * fdgpu_debug_qm_first_insertions: first insertion wins over hashes[max(n_cfg, 1)][n_cands], the insertions in (candidate, bin configuration)
 *   order (position = candidate * max(n_cfg, 1) + configuration): *keep = the kept positions, ascending.  table_max / set_min: the switches between the table, the radix
 *   and the hash-set form (0 = the library's 4,096 and 2^32).
 * fdgpu_debug_qm_arena: offsets[15] = byte offsets {hash, qi, qj, idf, primary_hash, post_len, post_kidx, post_seg, indices, aad_dist, aad_qi, is_primary,
 *   aad_aa1, aad_aa2} of a map's block and its size.
 * fdgpu_debug_qm_fill: one map (fdgpu_query_map_free) from kept positions and per-candidate / per-pair arrays: cand_recs != NULL = the host form's
 *   stored candidates, else candidate z is insertion z % per_pair of valid pair valid_pairs[z / per_pair]; post_len NULL = no posting arrays. */
int fdgpu_debug_qm_pairs(uint64_t n_queries, const uint32_t *q_struct, const uint64_t *q_off, const uint32_t *q_index, const uint64_t *res_off,
                         uint32_t **pair_i, uint32_t **pair_j, uint64_t *pair_off);
int fdgpu_debug_qm_fields(uint32_t hash_type, int32_t *out);
int fdgpu_debug_qm_expand(const float *features, const uint8_t *valid, const uint32_t *pair_i, const uint32_t *pair_j, uint64_t n_pairs, uint64_t r0,
                          const uint32_t *q_index, uint64_t n_q, const uint8_t *const *subs, const uint32_t *n_subs, uint32_t hash_type,
                          const float *dist_thr, uint64_t n_dist, const float *angle_thr_rad, uint64_t n_angle, float **cand_features,
                          uint32_t **cand_recs, uint64_t *n_cands);
int fdgpu_debug_qm_first_insertions(const uint32_t *hashes, uint64_t n_cands, uint32_t n_cfg, uint64_t table_max, uint64_t set_min, uint32_t **keep,
                                    uint64_t *n_keep);
int fdgpu_debug_qm_arena(uint64_t n, uint64_t n_indices, uint64_t n_aad, uint32_t with_post, uint64_t *offsets);
int fdgpu_debug_qm_fill(const uint32_t *keep, uint64_t n, const uint32_t *hashes, uint64_t n_cands, uint32_t n_cfg, uint64_t c0, const uint32_t *cand_recs,
                        const uint32_t *valid_pairs, uint64_t per_pair, const uint32_t *pair_i, const uint32_t *pair_j, uint64_t r0, const float *pair_idf,
                        const uint32_t *pair_primary, const uint64_t *post_len, const uint32_t *post_seg, const long long *post_kidx, uint64_t index_uid,
                        const uint32_t *indices, uint64_t n_indices, const uint8_t *aad_aa1, const uint8_t *aad_aa2, const float *aad_dist,
                        const uint32_t *aad_qi, uint64_t n_aad, uint32_t pooled, fd_query_map **out);

#ifdef __cplusplus
}
#endif
#endif
