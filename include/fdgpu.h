/* fdgpu.h — C ABI of libfdgpu.so, the MI355X (gfx950) implementation of Folddisco's
 * geometric-hash index-build and motif-query hot path.
 *
 * The reference (steineggerlab/folddisco, Rust) has no FFI for this path; its call seams
 * are plain Rust functions.  Each entry point below replaces one seam and
 * is what a `#[link(name = "fdgpu")] extern "C"` block in the reference would bind
 * (INTEGRATION.md shows the Rust side).  Conventions follow the one FFI precedent in the
 * reference, Foldcomp (lib/foldcomp/foldcompffi.h:8-21, src/structure/io/fcz.rs:82-93):
 * opaque handles, borrowed inputs, malloc'd outputs owned by the caller and released with
 * fdgpu_free().  Unlike Foldcomp nothing aborts: every call returns 0 or a negative
 * FDGPU_E* code and fdgpu_last_error() gives the text.
 *
 * All pointers are plain host pointers unless a parameter says "device".  No torch types.
 */
#ifndef FDGPU_H
#define FDGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDGPU_OK 0
#define FDGPU_EINVAL (-1)   /* bad argument */
#define FDGPU_EHIP (-2)     /* HIP runtime error (no device, launch failure, OOM) */
#define FDGPU_ENOMEM (-3)   /* host allocation failed */
#define FDGPU_ERANGE (-4)   /* size limit exceeded (e.g. structure > 65535 residues) */

typedef struct fdgpu_ctx fdgpu_ctx;       /* one per GPU / HIP stream */
typedef struct fdgpu_batch fdgpu_batch;   /* packed structures resident in HBM */
typedef struct fdgpu_index fdgpu_index;   /* inverted index resident in HBM */

/* ---- context ------------------------------------------------------------------------- */
/* fdgpu_create runs a start-up self-check (FDGPU_SELFCHECK=0 skips it): the six 4CHA triad hashes the reference's own test holds
 * (src/controller/graph.rs:71-79) through every evaluation path of the pair kernel — a mismatch fails with FDGPU_EHIP — and a probe of
 * the HOST's libm against the glibc generation the device arithmetic restates (fdgpu_host_libm_matches). */
int fdgpu_create(int device, fdgpu_ctx **out);
/* 1: this host's sinf/cosf/acosf/atan2f agree with the restated generation (a reference build here hashes like this library),
 * 0: they differ (warning on stderr), -1: self-check skipped */
int fdgpu_host_libm_matches(const fdgpu_ctx *ctx);
void fdgpu_destroy(fdgpu_ctx *ctx);
/* use an existing hipStream_t (e.g. torch's current stream); NULL = the context's own stream */
int fdgpu_set_stream(fdgpu_ctx *ctx, void *hip_stream);
int fdgpu_synchronize(fdgpu_ctx *ctx);
/* Returns the context's workspaces (an index build keeps 12 bytes per key of its largest call: 80 GB after a 203,250-structure call, 213 GB
 * after Swiss-Prot in one call) and the cached device blocks of destroyed indices to the device.  Indices, batches and query maps stay valid.
 * (No reference counterpart: the reference's builder frees its DashMap / Vec buffers when they go out of scope, src/cli/workflows/build_index.rs.) */
int fdgpu_release_workspaces(fdgpu_ctx *ctx);
const char *fdgpu_last_error(const fdgpu_ctx *ctx);
void fdgpu_free(void *host_ptr);
const char *fdgpu_version(void);

/* ---- packed structures --------------------------------------------------------------------
 * One batch = one rayon chunk of the reference (src/controller/mod.rs:282-348).  Residue k of
 * structure s lives at r = res_off[s] + k.  This is CompactStructure
 * (src/structure/core.rs:56-67) flattened: coordinates interleaved x,y,z as f32. */
typedef struct fd_batch_desc {
    uint64_t n_struct;
    const uint64_t *res_off;   /* [n_struct+1], res_off[0] = 0 */
    const float *n_xyz;        /* [3*R] backbone N  */
    const float *ca_xyz;       /* [3*R] C-alpha     */
    const float *cb_xyz;       /* [3*R] C-beta (real or approx_cb virtual); ignored where !cb_valid */
    const uint8_t *aa;         /* [R] map_aa_to_u8 (src/utils/convert.rs:53-81): 0..19, 255 = unknown */
    const uint8_t *cb_valid;   /* [R] 1 if CB is Some (src/structure/core.rs:147-155); NULL = all 1 */
} fd_batch_desc;

/* Parameters of the encoding.  hash_type = the reference's HashType index (src/geometry/core.rs:26-40), all nine built:
 * 3 PDBTrRosetta (the default, pdb_tr.rs:21-75; the fast table / speculative path) and, over the same
 * (d_CA, d_CB, theta, tau1, tau2) descriptor, 0 PDBMotif (pdb_motif.rs), 1 PDBMotifSinCos (pdb_motif_sincos.rs),
 * 7 FolddiscoAngle (folddisco_angle.rs), 8 FolddiscoDist (folddisco_dist.rs); with their own descriptors (one ordered pair at a
 * time, exact libm, 32-bit hashes) 2 TrRosetta (trrosetta.rs), 4 PointPairFeature (ppf.rs), 5 TertiaryInteraction
 * (tertiary_interaction.rs), 6 Hybrid (hybrid.rs) — for those four fdgpu_hash_batch serves the raw order only, and
 * fdgpu_pair_features / fdgpu_hash_features (seven-float records) are not available.  Retrieval with 5 / 6 scans every residue
 * pair (the reference's amino-acid prefilter panics there for queries of <= 200 hashes).
 * nbin_dist / nbin_angle follow the reference: if either is 0 both take the encoding's defaults
 * (controller/feature.rs:216-223), larger values clamp per encoding. */
#define FDGPU_HASH_PDBMOTIF 0u
#define FDGPU_HASH_PDBMOTIF_SINCOS 1u
#define FDGPU_HASH_TRROSETTA 2u
#define FDGPU_HASH_PDBTR 3u
#define FDGPU_HASH_PPF 4u
#define FDGPU_HASH_TERTIARY 5u
#define FDGPU_HASH_HYBRID 6u
#define FDGPU_HASH_FOLDDISCO_ANGLE 7u
#define FDGPU_HASH_FOLDDISCO_DIST 8u
#define FDGPU_MAX_MULTIPLE_BINS 8
typedef struct fd_hash_params {
    uint32_t nbin_dist;
    uint32_t nbin_angle;
    float dist_cutoff;         /* CA-CA cutoff in Angstrom (strict >, src/structure/core.rs:391) */
    uint32_t hash_type;        /* FDGPU_HASH_*; NOTE 0 is PDBMotif, as in the reference's numbering: set FDGPU_HASH_PDBTR (3) for the default encoding */
    /* --multiple-bins d1-a1,d2-a2,... (src/cli/workflows/build_index.rs:45,149-153): every residue pair is hashed once per
     * (dist, angle) bin pair and all the hashes share one index (controller/feature.rs:211-215); queries insert every
     * expansion under every bin pair (controller/query.rs:59-70) and retrieval reports a found triple per matching bin pair
     * (controller/retrieve.rs:124-131).  0 = off.  Zero bin counts inside the list are rejected (the reference treats them
     * differently at index and at query time).  nbin_dist / nbin_angle above still select the observed hash that idf is
     * looked up for (query.rs:283-288).  Honoured by fdgpu_index_build, fdgpu_make_query_map[_batch], fdgpu_match_pairs and
     * fdgpu_retrieve[_batch]; fdgpu_hash_batch returns FDGPU_EINVAL with it. */
    uint32_t n_multiple_bins;
    uint32_t multiple_bins[FDGPU_MAX_MULTIPLE_BINS][2];
} fd_hash_params;

/* copy a host batch into HBM */
int fdgpu_batch_upload(fdgpu_ctx *ctx, const fd_batch_desc *host, fdgpu_batch **out);
/* wrap arrays that already live in HBM (all pointers in `dev` are device pointers; res_off too).
 * The memory is borrowed, not owned. */
int fdgpu_batch_wrap_device(fdgpu_ctx *ctx, const fd_batch_desc *dev, uint64_t total_residues,
                            fdgpu_batch **out);
void fdgpu_batch_destroy(fdgpu_batch *b);
uint64_t fdgpu_batch_num_structures(const fdgpu_batch *b);
uint64_t fdgpu_batch_num_residues(const fdgpu_batch *b);

/* ---- operations on a resident batch ------------------------------------------------------------------------
 * A resident database is an fdgpu_index and the fdgpu_batch of its coordinates.  Every id-mapping index operation has a batch counterpart, so
 * the pair stays addressable by the candidate ids scoring returns: fdgpu_index_remove(keep) ~ select of the kept ids in ascending order,
 * fdgpu_index_permute(new_id) ~ select of argsort(new_id), part r of fdgpu_index_split(bounds) ~ select of bounds[r] .. bounds[r + 1] - 1,
 * fdgpu_index_merge ~ fdgpu_batch_concat.  Bytes are copied verbatim.  The results own their memory (fdgpu_batch_destroy); the sources stay valid.
 *
 * fdgpu_batch_select: structure k of *out = structure ids[k] of b, in the order given — a gather: repeats are allowed, n = 0 gives an empty batch,
 * a source without cb_valid gives a result without it.  Checked on the host before anything is launched: an id >= the batch's structures is
 * FDGPU_EINVAL, a result of 2^32 residues or more FDGPU_ERANGE (the sum is 64-bit: repeats can reach it).  On any error *out is NULL. */
int fdgpu_batch_select(fdgpu_ctx *ctx, const fdgpu_batch *b, const uint32_t *ids, uint64_t n, fdgpu_batch **out);
/* the parts one after the other (2 .. 64 parts, a part may be empty; anything else FDGPU_EINVAL): device-to-device copies.  If only some parts
 * carry cb_valid the others contribute ones.  FDGPU_ERANGE for 2^32 residues or structures.  On any error *out is NULL. */
int fdgpu_batch_concat(fdgpu_ctx *ctx, const fdgpu_batch *const *parts, uint64_t n_parts, fdgpu_batch **out);
/* the five arrays and res_off of a resident batch back on the host: host_out is filled like the fd_batch_desc of fdgpu_batch_upload, every array
 * released with fdgpu_free; cb_valid = NULL where the batch has none. */
int fdgpu_batch_export(fdgpu_ctx *ctx, const fdgpu_batch *b, fd_batch_desc *host_out);

/* ---- S1: per-structure hashes -------------------------------------------------------------
 * Replaces get_geometric_hash_as_u32_from_structure (src/controller/feature.rs:198-231)
 * followed by the caller's sort_unstable(); dedup() (src/controller/mod.rs:343-345), for every
 * structure of the batch.  *hashes = concatenated sorted-unique lists, (*hash_off)[s] .. [s+1].
 * With sort_dedup = 0 the raw list in the reference's row-major pair order is returned. */
int fdgpu_hash_batch(fdgpu_ctx *ctx, const fdgpu_batch *b, const fd_hash_params *p, int sort_dedup,
                     uint32_t **hashes, uint64_t **hash_off);

/* The raw list WITH positions: entries [row_off[i], row_off[i + 1]) belong to residue i of the batch (row-major pair order), entry k
 * pairs it with residue partner[k] and hashes[k] is the pair's hash — the (hash, i, j) stream collect_hash_id_pos walks for
 * `analyze -p` (src/controller/summary.rs:632-690).  row_off has n_residues + 1 entries.  Release the three arrays with fdgpu_free. */
int fdgpu_hash_batch_rows(fdgpu_ctx *ctx, const fdgpu_batch *b, const fd_hash_params *p, uint32_t **hashes, uint32_t **partner, uint64_t **row_off);

/* ---- S2: inverted index build ----------------------------------------------------------------
 * Replaces Folddisco::collect_and_count + allocate_entries + add_entries +
 * wrapup_offset_and_save_entries + prune_to_sparse (src/controller/mod.rs:274-441,
 * src/index/indextable.rs:88-295) for the structures of `b`, which receive ids
 * first_id, first_id+1, ...  The result (value bytes, sparse hashes, offsets) stays in HBM.
 * One call of the default encoding holds up to 2^24 structures and 2^35 residue-pair keys and needs 12 bytes of workspace per key
 * (Swiss-Prot, 1.77e10 keys: 213 GB); FDGPU_ERANGE / FDGPU_EHIP (out of memory) beyond that: build consecutive id ranges and
 * fdgpu_index_merge them.  The other encodings and --multiple-bins: 2^32 keys per call. */
int fdgpu_index_build(fdgpu_ctx *ctx, const fdgpu_batch *b, const fd_hash_params *p, uint64_t first_id,
                      fdgpu_index **out);
/* copy the index to the host in the reference's on-disk layout:
 * value = PREFIX file, hashes/offsets = payload of PREFIX.offset. */
int fdgpu_index_export(fdgpu_ctx *ctx, const fdgpu_index *ix, uint8_t **value, uint64_t *value_len,
                       uint32_t **hashes, uint64_t **offsets, uint64_t *n_hashes);
/* upload an existing index (load_folddisco_index, src/index/indextable.rs:331-394).
 * nres[S] = per-structure residue counts from the .lookup file (length penalty). */
int fdgpu_index_load(fdgpu_ctx *ctx, const uint32_t *hashes, const uint64_t *offsets, uint64_t n_hashes,
                     const uint8_t *value, uint64_t value_len, uint64_t n_structures, fdgpu_index **out);
/* an uploaded index that is one shard of a database (structures first_id .. first_id + n_structures - 1, as written by a sharded
 * build): tells scoring and fdgpu_index_merge where the shard's ids start (0 after fdgpu_index_load).  This only LABELS the index: not a byte
 * of it changes, the ids inside the lists must already be the absolute ones.  fdgpu_index_rebase REWRITES the lists for another id range. */
int fdgpu_index_set_first_id(fdgpu_index *ix, uint64_t first_id);
void fdgpu_index_destroy(fdgpu_index *ix);
uint64_t fdgpu_index_num_hashes(const fdgpu_index *ix);
uint64_t fdgpu_index_value_len(const fdgpu_index *ix);
uint64_t fdgpu_index_num_postings(const fdgpu_index *ix);
uint64_t fdgpu_index_num_structures(const fdgpu_index *ix);   /* structures the index covers (ids first_id ...); a merged index: the sum over its parts */
/* write PREFIX and PREFIX.offset byte-identically to save_offset_to_file (indextable.rs:297-326) */
int fdgpu_index_save(fdgpu_ctx *ctx, const fdgpu_index *ix, const char *prefix);
/* optional: make the page-locked staging slots of fdgpu_index_save / _save_part / _export now (256 MB, ~20 ms) — e.g. while the first chunk is still parsed */
int fdgpu_reserve_staging(fdgpu_ctx *ctx);

/* ---- S3: posting-list scoring -----------------------------------------------------------------
 * posting-list lengths of query hashes: FolddiscoIndex::get_entries(h).len()
 * (indextable.rs:83-86) — what calculate_idf_for_hash (src/controller/query.rs:17-32) and
 * count_query (src/controller/count_query.rs:121-130) need for log2(S / len). */
int fdgpu_posting_lengths(fdgpu_ctx *ctx, const fdgpu_index *ix, const uint32_t *q_hash, uint64_t n_q,
                          uint64_t *lengths);

/* byte length of the posting lists (get_raw_entries(h).len(), indextable.rs:53-81): what a scoring pass reads — the
 * algorithmic-bytes figure of the query roofline; 0 for an absent hash */
int fdgpu_posting_bytes(fdgpu_ctx *ctx, const fdgpu_index *ix, const uint32_t *q_hash, uint64_t n_q, uint64_t *bytes);

typedef struct fd_count_rec {   /* one touched structure (StructureResult prefilter fields) */
    uint32_t nid;
    uint32_t total_match_count;
    uint32_t node_count;
    uint32_t edge_count;
    float idf;                  /* sum_hits log2(S/len) * nres^(-length_penalty) */
} fd_count_rec;

/* Replaces count_query (src/controller/count_query.rs:82-220), no sampling.
 * q_hash[k] belongs to query edge (q_node[k], q_edge_j[k]) (= first / second query residue).
 * q_idf[k] = log2(S / len(posting(q_hash[k]))) as computed by the caller (glibc log2f keeps the
 * reference's bits); hashes failing freq_filter must be dropped by the caller.
 * penalty[nid] = (nres[nid] as f32).powf(-lp) (count_query.rs:200), n_structures entries.
 * Results: touched structures in ascending nid. */
int fdgpu_count_query(fdgpu_ctx *ctx, const fdgpu_index *ix, const uint32_t *q_hash, const uint32_t *q_node,
                      const uint32_t *q_edge_j, const float *q_idf, uint64_t n_q, const float *penalty,
                      fd_count_rec **out, uint64_t *n_out);

/* get_entries (src/index/indextable.rs:83-86; varint decode :421-463) for n_q hashes at once: the structure ids of hash k are
 * (*ids)[(*ids_off)[k] .. (*ids_off)[k+1]) in ascending order (empty for an absent hash).  Release both with fdgpu_free. */
int fdgpu_get_entries(fdgpu_ctx *ctx, const fdgpu_index *ix, const uint32_t *q_hash, uint64_t n_q, uint32_t **ids, uint64_t **ids_off);

/* Batched form: n_queries queries scored in one set of launches.  Query t owns entries [q_off[t], q_off[t+1]) of the
 * concatenated q_* arrays; its results are (*out)[(*out_off)[t] .. (*out_off)[t+1]) (ascending nid). */
int fdgpu_count_query_batch(fdgpu_ctx *ctx, const fdgpu_index *ix, uint64_t n_queries, const uint64_t *q_off,
                            const uint32_t *q_hash, const uint32_t *q_node, const uint32_t *q_edge_j, const float *q_idf,
                            const float *penalty, fd_count_rec **out, uint64_t **out_off);

/* As above with the candidate selection of query_pdb.rs:404-411 done on the device: per query only the top_n records come back,
 * ranked as the reference ranks them (idf descending, ties by ascending nid) — radix selection of the cut-off, then a bitonic sort in
 * LDS, so top_n records per query cross the bus.  top_n = 0: everything, in ascending nid. */
int fdgpu_count_query_batch_top(fdgpu_ctx *ctx, const fdgpu_index *ix, uint64_t n_queries, const uint64_t *q_off,
                                const uint32_t *q_hash, const uint32_t *q_node, const uint32_t *q_edge_j, const float *q_idf,
                                const float *penalty, uint32_t top_n, fd_count_rec **out, uint64_t **out_off);
/* The length penalty nres^(-lp) of the index's structures (count_query.rs:200) kept on the device: fdgpu_count_query* may then be
 * called with penalty = NULL instead of uploading n_structures floats per call.  penalty = NULL drops the resident copy. */
int fdgpu_index_set_penalty(fdgpu_ctx *ctx, fdgpu_index *ix, const float *penalty);
/* count_query for the query maps fdgpu_make_query_map[_batch] returned, without a round trip through the caller: every entry
 * (hash, (qi, qj)) of every map is scored with idf = log2f(total_structures / posting length of the hash itself)
 * (count_query.rs:181-200; the idf stored in the map belongs to the pair's observed hash and feeds the subgraph idf of the retrieval),
 * hashes the index does not hold are dropped.  Output as fdgpu_count_query_batch_top (top_n = 0: everything, ascending nid).
 * fd_query_map is declared further down. */
struct fd_query_map;
int fdgpu_count_query_maps_top(fdgpu_ctx *ctx, const fdgpu_index *ix, uint64_t n_queries, const struct fd_query_map *const *qms,
                               const float *penalty, float total_structures, uint32_t top_n, fd_count_rec **out, uint64_t **out_off);


/* ---- S4: candidate matching + RMSD --------------------------------------------------------------
 * Pair scan of retrieve_with_prefilter (src/controller/retrieve.rs:52-156) over candidate
 * structures of a resident batch.  For candidate c = cand[k] every ordered residue pair (i,j)
 * that passes the CA cutoff, the amino-acid/CA-distance window test against the query's
 * observed (aa_i, aa_j, dist, qi) list and has a feature is a "candidate pair"; those whose
 * hash is in the (sorted) query hash set are "found" triples. */
typedef struct fd_pair_rec { uint32_t cand; uint32_t i; uint32_t j; uint32_t hash; } fd_pair_rec;
typedef struct fd_cand_rec { uint32_t cand; uint32_t qi; uint32_t i; uint32_t j; } fd_cand_rec;
typedef struct fd_match_query {
    const uint32_t *hashes;     /* sorted unique query hashes */
    uint64_t n_hashes;
    const uint8_t *aad_aa1, *aad_aa2;   /* observed_distance_map flattened (query.rs:271-281) */
    const float *aad_dist;
    const uint32_t *aad_qi;
    uint64_t n_aad;
    float ca_distance_cutoff;   /* --ca-distance, default 1.0 */
    int use_aa_prefilter;       /* prefilter_amino_acid active (<= 200 query hashes, retrieve.rs:569) */
} fd_match_query;
/* resname_std[r] = 1 if the residue's 3-letter name equals map_u8_to_aa(aa) (retrieve.rs:580-586);
 * needed only when use_aa_prefilter. Pass NULL to treat every residue with aa < 20 as standard. */
int fdgpu_match_pairs(fdgpu_ctx *ctx, const fdgpu_batch *db, const uint8_t *resname_std,
                      const uint32_t *cand, uint64_t n_cand, const fd_match_query *q, const fd_hash_params *p,
                      fd_pair_rec **found, uint64_t *n_found, fd_cand_rec **cands, uint64_t *n_cands);

/* Batched Kabsch (src/structure/kabsch.rs:157-554, mode 2): problem k superposes
 * x[off[k]..off[k+1]) (moving = target points) onto y[...] (fixed = query points);
 * points are xyz f32.  rmsd[k] f32, rot[9k..], tran[3k..]. */
int fdgpu_kabsch_batch(fdgpu_ctx *ctx, const float *x, const float *y, const uint64_t *off, uint64_t n_problems,
                       float *rmsd, float *rot, float *tran);
/* Similarity metrics of n superpositions on the device (src/structure/metrics.rs:62-251 applied to KabschSuperimposer's reference /
 * transformed coordinates, kabsch.rs:86-95,145-154): problem k compares the fixed points ref[off[k] .. off[k+1]) with
 * rot[9k ..] * mov[...] + tran[3k ..] (f32, as matrix_vector_multiply + add_vec do).  metrics[5k ..] = tm_score, gdt_ts, gdt_ha,
 * chamfer_distance, hausdorff_distance — what --tm-score / --gdt-ts / --gdt-ha / --chamfer / --hausdorff filter and sort on. */
int fdgpu_metrics_batch(fdgpu_ctx *ctx, const float *ref, const float *mov, const uint64_t *off, uint64_t n_problems, const float *rot,
                        const float *tran, float *metrics);
/* Batched partial fit = LmsQcpSuperimposer::new() + set_atoms(fixed = y, moving = x) + run() with the default parameters
 * (src/structure/lms_qcp.rs:29-41, 91-249; what --partial-fit selects for matches of more than 3 residues,
 * src/controller/retrieve.rs:733-746): rmsd[k] = rms over the final core, rot/tran map x onto y.  Every problem needs
 * >= 3 pairs.  Optional: core_len[k] = size of the core, core[off[k] .. off[k] + core_len[k]) = its pair indices in
 * joining order. */
int fdgpu_lms_qcp_batch(fdgpu_ctx *ctx, const float *x, const float *y, const uint64_t *off, uint64_t n_problems,
                        float *rmsd, float *rot, float *tran, uint32_t *core_len, uint32_t *core);

/* ---- query map and retrieval (host glue in C++, numerics on the GPU) ------------------------------------
 * get_single_feature (src/controller/feature.rs:11-24, 84-99) for explicit residue pairs (i, j) of
 * structure s of a batch: features[k] = {aa_i, aa_j, d_CA, d_CB, theta, tau1, tau2}, valid[k] = has a feature. */
int fdgpu_pair_features(fdgpu_ctx *ctx, const fdgpu_batch *b, uint64_t s, const uint32_t *pair_i, const uint32_t *pair_j,
                        uint64_t n, const fd_hash_params *p, float *features /*[n][7]*/, uint8_t *valid);
/* GeometricHash::perfect_hash (src/geometry/pdb_tr.rs:21-75) on explicit 7-float feature vectors */
int fdgpu_hash_features(fdgpu_ctx *ctx, const float *features, uint64_t n, const fd_hash_params *p, uint32_t *hashes);

typedef struct fd_query_map {   /* make_query_map output (src/controller/query.rs:208-329), first-insertion order */
    uint64_t n;
    uint32_t *hash; uint32_t *qi; uint32_t *qj; uint8_t *is_primary; float *idf;
    uint64_t n_indices; uint32_t *indices;                 /* all_query_indices */
    uint64_t n_aad; uint8_t *aad_aa1; uint8_t *aad_aa2; float *aad_dist; uint32_t *aad_qi;   /* observed_distance_map */
    uint32_t *primary_hash;     /* [n] observed hash of the residue pair entry k belongs to: idf[k] = log2(S / posting length of it)
                                 * — lets a caller that shards the index recompute idf from GLOBAL posting lengths */
    /* set by the library when the map was made against an index (private to it, may be NULL): the posting length and the number of
     * 2 KB scoring segments of every entry's OWN hash in that index — fdgpu_count_query_maps_top then scores without a second
     * posting-length pass and without asking the device for its work count */
    uint64_t *post_len; uint32_t *post_seg; uint64_t post_index_uid;
    long long *post_kidx;       /* with post_len: position of every entry's hash in that index's hash array (-1: absent) — scoring skips its own search */
    uint64_t arena_bytes;       /* private: non-zero when the struct and every array above are ONE allocation of that size (release only through fdgpu_query_map_free) */
} fd_query_map;
/* qb = batch holding the query structure as structure 0; q_index[k] = residue index of the k-th query
 * residue (after parse_query_string + get_index / --serial-index resolution on the caller's side);
 * subs[k] = amino-acid substitution list of residue k or NULL; thresholds as given to -d / -a (angles in
 * degrees); index may be NULL (idf 0). */
int fdgpu_make_query_map(fdgpu_ctx *ctx, const fdgpu_batch *qb, const uint32_t *q_index, uint64_t n_q,
                         const uint8_t *const *subs, const uint32_t *n_subs, const float *dist_thr, uint64_t n_dist,
                         const float *angle_thr_deg, uint64_t n_angle, const fd_hash_params *p, const fdgpu_index *index,
                         float total_structures, fd_query_map **out);
/* Many queries, three launches in total: query t = structure q_struct[t] of qb with residues q_index[q_off[t] .. q_off[t+1]);
 * subs / n_subs run parallel to q_index (may be NULL); out[t] per query, each released with fdgpu_query_map_free. */
int fdgpu_make_query_map_batch(fdgpu_ctx *ctx, const fdgpu_batch *qb, uint64_t n_queries, const uint32_t *q_struct, const uint64_t *q_off,
                               const uint32_t *q_index, const uint8_t *const *subs, const uint32_t *n_subs, const float *dist_thr,
                               uint64_t n_dist, const float *angle_thr_deg, uint64_t n_angle, const fd_hash_params *p,
                               const fdgpu_index *index, float total_structures, fd_query_map **out);
void fdgpu_query_map_free(fd_query_map *m);

typedef struct fd_match_rec {   /* one connected component of one candidate (retrieval_wrapper, retrieve.rs:364-552) */
    uint32_t cand;              /* slot in the candidate list */
    uint32_t same;              /* processed mapping == from-hash mapping */
    float idf;                  /* subgraph idf */
    float rmsd;                 /* of the processed mapping (what the per-match output prints) */
    float rmsd_from_hash;
    float rot[9], tran[3];      /* target -> query superposition of the processed mapping */
    float metrics[5];           /* tm_score, gdt_ts, gdt_ha, chamfer, hausdorff of that superposition (structure/metrics.rs) */
    float rot_from_hash[9], tran_from_hash[3], metrics_from_hash[5];   /* the same for the from-hash mapping (--skip-ca-match prints it) */
} fd_match_rec;
/* residues: 2 * n_indices int32 per match — target residue index (relative to its structure, -1 = "_") for
 * every query residue, first the from-hash mapping then the processed (rescued) one. Release both with
 * fdgpu_matches_free. Matches are ordered by candidate slot, then by component as in graph.rs:43-45.
 * partial_fit != 0 = --partial-fit: mappings of more than 3 residues are superposed by the least-median-of-squares
 * fit (fdgpu_lms_qcp_batch) and report the rms over its core (retrieve.rs:733-746, 787-812). */
int fdgpu_retrieve(fdgpu_ctx *ctx, const fdgpu_batch *db, const uint8_t *resname_std, const uint32_t *cand, uint64_t n_cand,
                   const fd_query_map *qm, const fdgpu_batch *qb, const fd_hash_params *p, float ca_distance_cutoff,
                   uint32_t node_count, uint32_t partial_fit, fd_match_rec **matches, uint64_t *n_matches, int32_t **residues);
/* Many queries with one pair scan, one coordinate gather and one Kabsch launch in total: query t = structure q_struct[t] of qb
 * with the query map qms[t]; its candidates are cand[cand_off[t] .. cand_off[t+1]).  Matches of query t =
 * (*matches)[(*match_off)[t] .. (*match_off)[t+1]) (cand = slot inside the query's own list), its residues start at
 * (*residues)[(*res_off)[t]], 2 * qms[t]->n_indices per match.  Release matches/residues with fdgpu_matches_free, the two
 * offset arrays with fdgpu_free. */
int fdgpu_retrieve_batch(fdgpu_ctx *ctx, const fdgpu_batch *db, const uint8_t *resname_std, uint64_t n_queries, const uint32_t *cand,
                         const uint64_t *cand_off, const fd_query_map *const *qms, const fdgpu_batch *qb, const uint32_t *q_struct,
                         const fd_hash_params *p, float ca_distance_cutoff, uint32_t node_count, uint32_t partial_fit,
                         fd_match_rec **matches, uint64_t **match_off, int32_t **residues, uint64_t **res_off);
void fdgpu_matches_free(fd_match_rec *m, int32_t *residues);
/* The per-query body of the query workflow (src/cli/workflows/query_pdb.rs:376-452: make_query_map -> count_query -> sort / truncate ->
 * retrieval_wrapper over the first candidates) for a rayon chunk of queries in ONE call: arguments as fdgpu_make_query_map_batch (queries),
 * fdgpu_count_query_maps_top (penalty NULL = the index's resident one, top_n ranked records per query) and fdgpu_retrieve_batch over the first
 * match_top records of every query's ranking (candidates = nid - the index's first id: db holds the index's structures in order).  Outputs
 * are exactly those of the three calls made one after the other: maps[t] (caller's array of n_queries pointers, each released with
 * fdgpu_query_map_free), recs / rec_off, matches / match_off / residues / res_off (fdgpu_free).  What the single call adds is overlap: the
 * retrieval's tables are built while the scoring kernels run and the ranked records cross the bus while the retrieval runs. */
int fdgpu_query_batch(fdgpu_ctx *ctx, const fdgpu_index *index, const fdgpu_batch *db, const uint8_t *resname_std, const fdgpu_batch *qb, uint64_t n_queries,
                      const uint32_t *q_struct, const uint64_t *q_off, const uint32_t *q_index, const uint8_t *const *subs, const uint32_t *n_subs,
                      const float *dist_thr, uint64_t n_dist, const float *angle_thr_deg, uint64_t n_angle, const fd_hash_params *p, float total_structures,
                      const float *penalty, uint32_t top_n, uint32_t match_top, float ca_distance_cutoff, uint32_t node_count, fd_query_map **maps,
                      fd_count_rec **recs, uint64_t **rec_off, fd_match_rec **matches, uint64_t **match_off, int32_t **residues, uint64_t **res_off);
/* The same call, NON-BLOCKING: submit hands the batch to one of the context's query LANES and returns, wait collects it.  The reference keeps
 * many queries in flight from its rayon workers (src/cli/workflows/query_pdb.rs:348 `queries.into_par_iter()`, :415 the retrieval's
 * par_iter_mut); a host with ONE thread per GPU gets that overlap here: submit batches k, k + 1, k + 2, then wait for k, submit k + 3, ... — a
 * lane is a private sibling context (own HIP stream, workspaces, landing blocks) driven by a library thread through fdgpu_query_batch itself, so
 * one batch's host-side steps (table building, waits for counts, result copies) are covered by the other lanes' kernels, and the results are bit
 * for bit those of the blocking call.  Lanes are made on the first submit (default 6, env FDGPU_QUERY_LANES, or fdgpu_query_lanes beforehand;
 * each lane holds its own query scratch in HBM — ~1 GB for batches of 128 queries at 542,000 structures) and are torn down by fdgpu_destroy.
 * Inputs: the per-query arrays (q_struct, q_off, q_index, subs, n_subs, thresholds, *p) are COPIED at submit; index, db, qb, resname_std and
 * penalty are borrowed until the wait returns.  Every submitted job must be waited for exactly once (that releases it); passing NULL output
 * pointers to wait discards the results.  Errors of the batch are returned by wait (message in fdgpu_last_error(ctx)).  Submit and wait may
 * be called from different threads; jobs complete in any order. */
typedef struct fdgpu_query_job fdgpu_query_job;
int fdgpu_query_batch_submit(fdgpu_ctx *ctx, const fdgpu_index *index, const fdgpu_batch *db, const uint8_t *resname_std, const fdgpu_batch *qb, uint64_t n_queries,
                             const uint32_t *q_struct, const uint64_t *q_off, const uint32_t *q_index, const uint8_t *const *subs, const uint32_t *n_subs,
                             const float *dist_thr, uint64_t n_dist, const float *angle_thr_deg, uint64_t n_angle, const fd_hash_params *p, float total_structures,
                             const float *penalty, uint32_t top_n, uint32_t match_top, float ca_distance_cutoff, uint32_t node_count, fdgpu_query_job **job);
int fdgpu_query_batch_wait(fdgpu_ctx *ctx, fdgpu_query_job *job, fd_query_map **maps, fd_count_rec **recs, uint64_t **rec_off, fd_match_rec **matches,
                           uint64_t **match_off, int32_t **residues, uint64_t **res_off);
/* make sure the context has at least n_lanes lanes (1..8) -> the number it has, or a negative error code; n_lanes = 0 only reports */
int fdgpu_query_lanes(fdgpu_ctx *ctx, uint32_t n_lanes);
/* Result arrays of the query entry points come from a recycling pool (fdgpu_free puts them back; at most 256 MB of idle blocks are kept,
 * env FDGPU_OUT_POOL_MB overrides, 0 = keep nothing).  fdgpu_trim releases the idle blocks — page-locked ones included — e.g. after a burst of
 * large batches; the last fdgpu_destroy of the process does it too. */
void fdgpu_trim(void);

/* ---- multi-GPU query path (one process per GPU, RCCL over xGMI) ----------------------------------------------------
 * The index and the coordinates are sharded by structure id (every rank holds the postings and coordinates of its own id range,
 * fdgpu_index_build with first_id or fdgpu_index_load + fdgpu_index_set_first_id).  What the reference's query workflow
 * (src/cli/workflows/query_pdb.rs:376-452) would call instead of the single-index count_query / retrieval: rank 0 creates a unique id and
 * hands it to the other ranks by any means (file, MPI, env), every rank calls fdgpu_comm_init on its own context / GPU, then per batch of
 * queries fdgpu_sharded_count_query[_maps] and fdgpu_sharded_retrieve.  RCCL is bound at run time (dlopen); without it these calls return
 * FDGPU_EHIP.  The collectives are issued for every world size, one included.  A rank whose LOCAL STEP fails (posting lengths, scoring,
 * retrieval) still takes part in the call's collectives (zeros in the sum, its status in the gathered message) and every rank returns an
 * error: no rank is left waiting.  The exchange buffers of ordinary calls are reserved at fdgpu_comm_init.  A rank that cannot grow them
 * beyond that reserve, or whose HIP runtime fails between two collectives of a call, aborts the communicator (ncclCommAbort) and returns
 * FDGPU_EHIP: the communicator is then unusable on every rank (later calls fail at once) and must be created anew. */
#define FDGPU_COMM_ID_BYTES 128
typedef struct fdgpu_comm fdgpu_comm;
int fdgpu_comm_unique_id(uint8_t id[FDGPU_COMM_ID_BYTES]);
int fdgpu_comm_init(fdgpu_ctx *ctx, const uint8_t id[FDGPU_COMM_ID_BYTES], int rank, int world, fdgpu_comm **out);
void fdgpu_comm_destroy(fdgpu_comm *comm);
int fdgpu_comm_rank(const fdgpu_comm *comm);
int fdgpu_comm_world(const fdgpu_comm *comm);
/* collectives this communicator has issued so far (ncclAllReduce / ncclAllGather calls) */
int fdgpu_comm_stats(const fdgpu_comm *comm, uint64_t *n_allreduce, uint64_t *n_allgather);

/* ---- ONE on-disk index from N ranks, without the host (Option A) -----------------------------------------------
 * After a build sharded by structure every rank holds the resident sub-index of its id range; the reference's output contract is one
 * PREFIX / PREFIX.offset in ascending hash order (src/index/indextable.rs:239-326).  The hash space is cut into N ranges of about equal
 * posting bytes, every rank slices its sub-index at those bounds, piece j travels to rank j device to device, rank j concatenates the N
 * pieces of its range per hash on the device (fdgpu_index_merge: id ranges ascend with the source rank) and writes its regions of the two
 * files — byte-identical to the single-GPU build, because lists are (hash ascending, id ascending) either way.
 *   fdgpu_index_range_bounds   n_ranges - 1 ascending hash values cutting `index` into ranges of about equal posting bytes (range j holds
 *                              bounds[j - 1] <= hash < bounds[j]; one rank computes them, all ranks must use the same)
 *   fdgpu_index_slice          the lists with hash_lo <= hash < hash_hi (hash_hi up to 2^32) as a resident index of their own (same id range)
 *   fdgpu_comm_single_index    the whole exchange over RCCL (bounds from rank 0, slices, ncclSend / ncclRecv of piece j to rank j, merge):
 *                              -> this rank's hash range of the database's index and its place in it
 *   fdgpu_index_save_part      writes a range's regions of PREFIX / PREFIX.offset (see fd_shard_index.hip); ranks of one node may call it
 *                              concurrently; write_header != 0 on the rank of the first range, is_last != 0 on the rank of the last one
 * Hosts with another transport (MPI, gloo) use range_bounds + slice + fdgpu_index_export / _load + fdgpu_index_merge + save_part. */
int fdgpu_index_range_bounds(fdgpu_ctx *ctx, const fdgpu_index *index, uint32_t n_ranges, uint32_t *bounds);
int fdgpu_index_slice(fdgpu_ctx *ctx, const fdgpu_index *index, uint64_t hash_lo, uint64_t hash_hi, fdgpu_index **out);
int fdgpu_comm_single_index(fdgpu_ctx *ctx, fdgpu_comm *comm, const fdgpu_index *local, fdgpu_index **range_index, uint64_t *hashes_before,
                            uint64_t *value_before, uint64_t *total_hashes, uint64_t *total_value);
int fdgpu_index_save_part(fdgpu_ctx *ctx, const fdgpu_index *part, const char *prefix, uint64_t hashes_before, uint64_t value_before,
                          uint64_t total_hashes, uint64_t total_value, int write_header, int is_last);
/* lengths[k] <- sum over the ranks (ncclAllReduce): posting lengths of a shard -> posting lengths over the whole database, the
 * denominator of idf = log2(S / len) (src/controller/query.rs:17-32, count_query.rs:130) */
int fdgpu_allreduce_lengths(fdgpu_ctx *ctx, fdgpu_comm *comm, uint64_t *lengths, uint64_t n);
/* count_query of a batch of queries against the sharded index: every rank passes the same queries (layout of
 * fdgpu_count_query_batch, no idf: it is computed here from the posting lengths all-reduced on the device, with log2f) and its own shard +
 * penalty (one entry per structure of the shard; NULL = the resident copy of fdgpu_index_set_penalty).  The ranks score locally, select
 * their top_n on the device, all-gather selection state + ranked records in one device-to-device ncclAllGather and select / rank the union
 * on the device: per query (*out)[(*out_off)[t] .. (*out_off)[t+1]) = the global ranking (idf descending, nid ascending;
 * query_pdb.rs:404-411) truncated to top_n, identical on every rank.  nid = global structure id.  top_n = 0 (every touched structure)
 * and top_n > 3072 exchange variable-length lists instead (counts, then one padded payload) and rank on the host. */
int fdgpu_sharded_count_query(fdgpu_ctx *ctx, fdgpu_comm *comm, const fdgpu_index *ix, uint64_t n_queries, const uint64_t *q_off,
                              const uint32_t *q_hash, const uint32_t *q_node, const uint32_t *q_edge_j, const float *penalty,
                              uint64_t total_structures, uint32_t top_n, fd_count_rec **out, uint64_t **out_off);
/* The same for the query maps of fdgpu_make_query_map[_batch] (made with index = NULL): the sharded sibling of
 * fdgpu_count_query_maps_top.  One all-reduce carries the posting lengths of every map's hash[] (scoring idf) and primary_hash[]; the
 * maps' idf[] — the retrieval's subgraph idf (query.rs:283-288) — is REWRITTEN in place from the global lengths, so the maps can go on to
 * fdgpu_sharded_retrieve. */
int fdgpu_sharded_count_query_maps(fdgpu_ctx *ctx, fdgpu_comm *comm, const fdgpu_index *ix, uint64_t n_queries, fd_query_map *const *qms,
                                   const float *penalty, uint64_t total_structures, uint32_t top_n, fd_count_rec **out, uint64_t **out_off);
/* Retrieval against sharded coordinates (the candidate loop of query_pdb.rs:415-452): query t's candidates
 * cand_nid[cand_off[t] .. cand_off[t+1]) are GLOBAL structure ids in ranking order, the same on every rank; `db` holds the structures
 * first_id .. first_id + n - 1 of this rank.  Every candidate is matched on the rank that owns it, the match records and residue lists
 * are all-gathered (counts, then one padded payload) and merged by candidate slot: the output equals fdgpu_retrieve_batch over the whole
 * database with cand = the global lists (fd_match_rec.cand = slot in the query's list), identical on every rank.  Release like
 * fdgpu_retrieve_batch's outputs. */
int fdgpu_sharded_retrieve(fdgpu_ctx *ctx, fdgpu_comm *comm, const fdgpu_batch *db, uint64_t first_id, const uint8_t *resname_std,
                           uint64_t n_queries, const uint32_t *cand_nid, const uint64_t *cand_off, const fd_query_map *const *qms,
                           const fdgpu_batch *qb, const uint32_t *q_struct, const fd_hash_params *p, float ca_distance_cutoff,
                           uint32_t node_count, uint32_t partial_fit, fd_match_rec **matches, uint64_t **match_off, int32_t **residues,
                           uint64_t **res_off);
/* For hosts with their own transport (MPI, gloo): the two local halves of fdgpu_sharded_count_query_maps.  fdgpu_query_maps_lengths
 * writes the LOCAL posting lengths of all maps' hash[] (sum(n) values, maps in order) followed by all maps' primary_hash[] (sum(n) more);
 * the caller sums the 2 * sum(n) values over the ranks and hands them to fdgpu_count_query_maps_top_global, which rewrites the maps' idf[]
 * and scores the local shard (output as fdgpu_count_query_maps_top: this rank's top_n, ranked). */
int fdgpu_query_maps_lengths(fdgpu_ctx *ctx, const fdgpu_index *ix, uint64_t n_queries, const fd_query_map *const *qms, uint64_t *lengths);
int fdgpu_count_query_maps_top_global(fdgpu_ctx *ctx, const fdgpu_index *ix, uint64_t n_queries, fd_query_map *const *qms,
                                      const uint64_t *global_lengths, const float *penalty, float total_structures, uint32_t top_n,
                                      fd_count_rec **out, uint64_t **out_off);
/* The per-rank message of the device exchange: {u32 status, n_queries, top_n, cap} | {u32 x3, u32 count}[n_queries] |
 * fd_count_rec[n_queries][top_n], padded to 16 bytes (include/fdgpu_debug.h: the post-gather merges on hand-made messages).  0 < top_n <= 3072. */
uint64_t fdgpu_comm_message_bytes(uint64_t n_queries, uint32_t top_n);

/* ---- structure ingest (host, multi-threaded) ---------------------------------------------------------------
 * PDB / mmCIF text (optionally gzip) -> the packed arrays of fd_batch_desc plus what the .lookup file and the result
 * printer need.  Replaces read_structure_from_path + CompactStructure::build inside the index / query workflows
 * (src/controller/io.rs, src/structure/io/pdb.rs:37-77, src/structure/io/cif.rs:102-296, src/structure/core.rs:70-214,
 * quirks kept).  A structure with more than max_residue residues (0 = no limit) keeps its slot but has no residues and
 * pLDDT 0 (src/controller/mod.rs:313-318); an unreadable file has ok = 0 and no residues.  Format by file name:
 * *.cif / *.mmcif (+ .gz) = mmCIF, everything else = PDB.  Release with fdgpu_parsed_free. */
typedef struct fd_parsed {
    uint64_t n_struct, n_res;
    uint64_t *res_off;               /* [n_struct + 1] */
    float *n_xyz, *ca_xyz, *cb_xyz;  /* [3 * n_res] */
    uint8_t *aa, *cb_valid;          /* [n_res] 0..19 / 255; 1 = CB present (measured or virtual) */
    uint8_t *chain;                  /* [n_res] chain id (of the next residue's first atom, core.rs:116) */
    uint8_t *resname_std;            /* [n_res] 1 = the residue name is the standard 3-letter code of `aa` */
    uint64_t *serial;                /* [n_res] residue number */
    float *bfac;                     /* [n_res] */
    char *resname;                   /* [3 * n_res] */
    uint64_t *nres_raw;              /* [n_struct] residue count of the raw atom list (what max_residue is compared with) */
    float *plddt;                    /* [n_struct] mean b-factor, f32 sequential sum (core.rs:450-456) */
    uint8_t *ok;                     /* [n_struct] */
    uint8_t *first_chain;            /* [n_struct] chain id of the first atom (default chain of a query string) */
} fd_parsed;
int fdgpu_parse_structures(const char *const *paths, uint64_t n, uint32_t n_threads, uint64_t max_residue, fd_parsed **out);
void fdgpu_parsed_free(fd_parsed *p);
/* thread-seconds the ingest spent so far (summed over the threads of all fdgpu_parse_structures calls of the process): out[0] read + inflate,
 * out[1] text -> atom records, out[2] CompactStructure::build, out[3] files, out[4] inflated bytes; reset != 0 clears the counters */
void fdgpu_ingest_stats(double out[5], int reset);

/* Foldcomp input (reference: src/structure/io/fcz.rs — FoldcompDbReader::new :41-74, read_single_structure_by_id :203-230,
 * and the vendored decoder behind foldcomp_process, lib/foldcomp/foldcompffi.cpp).  fdgpu_foldcomp_decode turns one database
 * entry into the atom records the reference's Structure::update receives (coordinates bit-identical to the vendored decoder's:
 * backbone rebuilt from the stored torsion/bond angles forward and backward between anchors, O / CB / side chain placed from
 * them; atoms past CB carry their names but no coordinates — nothing on this path reads them).  fdgpu_foldcomp_db_list gives the
 * entries of DB.index in ascending key order (keys = the db_key column of the index's .lookup output; names from DB.lookup, joined
 * by '\n'; both released with fdgpu_free).  fdgpu_parse_foldcomp_db decodes the entries with the given keys (n_keys = 0: all, in
 * key order) and returns the same packed arrays as fdgpu_parse_structures. */
typedef struct fd_foldcomp_atom {
    float x, y, z, b;                /* coordinate, temperature factor (per-residue in Foldcomp) */
    char name[4];                    /* PDB-style padded atom name (" CA ", " OXT") */
    char res[3];                     /* residue name */
    uint8_t chain;
    uint64_t rser;                   /* residue serial: header.idx_residue + position */
} fd_foldcomp_atom;
int fdgpu_foldcomp_decode(const uint8_t *entry, uint64_t len, fd_foldcomp_atom **atoms, uint64_t *n_atoms);
int fdgpu_foldcomp_db_list(const char *db_path, uint64_t **keys, char **names, uint64_t *n_entries);
int fdgpu_parse_foldcomp_db(const char *db_path, const uint64_t *keys, uint64_t n_keys, uint32_t n_threads, uint64_t max_residue,
                            fd_parsed **out);

/* ---- merging per-GPU / per-batch sub-indices into the reference's single index ----------------------------
 * Parts must cover ascending, disjoint id ranges in the order given (index build shards by structure).  Output is
 * the on-disk layout (value bytes, sparse hashes, offsets[H+1]); host-side, buffers released with fdgpu_free. */
int fdgpu_merge_subindices(uint64_t n_parts, const uint8_t *const *values, const uint32_t *const *hashes,
                           const uint64_t *const *offsets, const uint64_t *n_hashes, uint8_t **out_value,
                           uint64_t *out_value_len, uint32_t **out_hashes, uint64_t **out_offsets, uint64_t *out_n_hashes);

/* The same merge on the device, for parts that are resident: a shard whose sort workspace does not fit one call is built as several
 * fdgpu_index_build calls over consecutive id ranges (the reference walks its input in chunks the same way,
 * src/controller/mod.rs:282-348) and the chunks' posting lists are concatenated per hash — first varint of every continuation
 * re-based to a delta — into ONE resident index, byte-identical to the index a single build over all the structures produces
 * (indextable.rs:171-202 appends ids in ascending order).  At most 64 parts per call; the parts stay valid. */
int fdgpu_index_merge(fdgpu_ctx *ctx, const fdgpu_index *const *parts, uint64_t n_parts, fdgpu_index **out);

/* Drop structures from a resident index.  keep[s] != 0 keeps structure first_id + s (n_keep == fdgpu_index_num_structures(ix)).
 * Kept structures are renumbered densely from first_id in their old order; lists that lose every id are dropped with their hash.
 * The result is byte-identical to fdgpu_index_build over the kept structures with the same first_id, carries per-list last ids
 * (so fdgpu_index_merge needs no extra decode pass), and leaves `ix` valid.  FDGPU_EINVAL if nothing is kept or n_keep mismatches.
 * Appending is fdgpu_index_build of the new structures at first_id + (kept count) and fdgpu_index_merge of the two. */
int fdgpu_index_remove(fdgpu_ctx *ctx, const fdgpu_index *ix, const uint8_t *keep, uint64_t n_keep, fdgpu_index **out);

/* Cut a resident index by structure id range, ids unchanged: the inverse of fdgpu_index_merge.  bounds[0 .. n_parts] ascend,
 * bounds[0] == first_id, bounds[n_parts] == first_id + n_structures (equal neighbours: an empty part), 1 <= n_parts <= 64; anything else is
 * FDGPU_EINVAL with nothing allocated.  out[r] holds, for every hash, the ids in [bounds[r], bounds[r+1]) (a hash without one is absent), with
 * first_id = bounds[r], n_structures = bounds[r+1] - bounds[r], exact posting counts and per-list last ids: byte-identical to fdgpu_index_build
 * over those structures with first_id = bounds[r], and fdgpu_index_merge of the parts in order gives `ix` back.  `ix` stays valid.  A decoded
 * id outside the index's range is FDGPU_EINVAL; on any error every part is destroyed and out[] is all NULL. */
int fdgpu_index_split(fdgpu_ctx *ctx, const fdgpu_index *ix, uint32_t n_parts, const uint64_t *bounds, fdgpu_index **out /* [n_parts] */);
/* The same cut on host arrays (the payload of PREFIX.offset and PREFIX), n_threads host threads over slot ranges (0 = 1).  No device.
 * Every out_* has n_parts entries; the arrays are released with fdgpu_free (out_offsets[r] has out_n_hashes[r] + 1 entries). */
int fdgpu_split_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t n_hashes, const uint8_t *value, uint64_t value_len, uint64_t first_id,
                     uint32_t n_parts, const uint64_t *bounds, uint32_t n_threads, uint8_t **out_value, uint64_t *out_value_len,
                     uint32_t **out_hashes, uint64_t **out_offsets, uint64_t *out_n_hashes);

/* Move a resident index to another id range: *out is a new resident index over the same structures with ids new_first_id ..
 * new_first_id + n_structures - 1, byte-identical to fdgpu_index_build over those structures with first_id = new_first_id (the first varint of
 * every list re-encoded, everything behind it moved), with the same hashes and posting count.  Rebase + fdgpu_index_merge joins indices that
 * were built separately, each with ids from 0; rebase to 0 of an fdgpu_index_split part makes the part a stand-alone index.  Per-list last ids:
 * shifted with the lists when `ix` carries them (a following fdgpu_index_merge then needs no decode pass); an index from fdgpu_index_load carries
 * none and neither does its rebased copy, exactly as if it had been loaded (merge, remove and split derive them on first use).  `ix` stays valid;
 * new_first_id == first_id gives a copy, an index without hashes an empty index (offsets == [0]).
 * FDGPU_ERANGE with nothing allocated when new_first_id + n_structures exceeds 32 bits (the limit of fdgpu_index_build and
 * fdgpu_index_set_first_id), FDGPU_ERANGE for a list that would reach 4 GiB, FDGPU_EINVAL for a damaged index (offsets that do not ascend inside
 * the value bytes, a first varint that leaves its list, a first id outside [first_id, first_id + n_structures)): all found before a byte is
 * written.  On any error *out is NULL. */
int fdgpu_index_rebase(fdgpu_ctx *ctx, const fdgpu_index *ix, uint64_t new_first_id, fdgpu_index **out);
/* The same move on host arrays (the payload of PREFIX.offset and PREFIX), n_threads host threads over slot ranges (0 = 1).  No device.  Same
 * bytes and same error codes as the device form (and FDGPU_EINVAL when first_id + n_structures exceeds 32 bits); the three arrays are released
 * with fdgpu_free (out_offsets has n_hashes + 1 entries, out_hashes is a copy of hashes). */
int fdgpu_rebase_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t n_hashes, const uint8_t *value, uint64_t value_len, uint64_t first_id,
                      uint64_t new_first_id, uint64_t n_structures, uint32_t n_threads, uint8_t **out_value, uint64_t *out_value_len,
                      uint32_t **out_hashes, uint64_t **out_offsets);

/* Reorder the structures of a resident index: new_id[k] = new local position of the structure now at local position k, a permutation of
 * 0 .. n - 1 with n == fdgpu_index_num_structures(ix).  *out is a new resident index over the same id range [first_id, first_id + n) that equals,
 * byte for byte, fdgpu_index_build over the same structures taken in the new order: the same hashes and posting count, every list decoded, mapped
 * (id -> first_id + new_id[id - first_id]), put back in ascending order and re-encoded, so offsets, value length and the per-list last ids (always
 * carried by the result) are new.  `ix` stays valid.  FDGPU_EINVAL, on the host and before any device work, when n differs from the index's number
 * of structures or new_id is not a permutation (a value >= n, a repeated value); FDGPU_EINVAL when a list holds an id outside
 * [first_id, first_id + n) or the offsets do not ascend inside the value bytes; FDGPU_ERANGE for a list of 4 GiB or more.  On any error *out is
 * NULL and nothing stays allocated.  Test switches, read per call, that only lower a class boundary of csrc/k_permute.hip: FDGPU_PERM_SORT_BYTES
 * (longest list sorted in LDS by one wavefront), FDGPU_PERM_LDS_BITS (most structures whose bitmap is kept in LDS). */
int fdgpu_index_permute(fdgpu_ctx *ctx, const fdgpu_index *ix, const uint32_t *new_id, uint64_t n, fdgpu_index **out);
/* The same reorder on host arrays (the payload of PREFIX.offset and PREFIX), n_threads host threads over slot ranges (0 = 1); n is the number of
 * structures.  No device.  Same bytes and same error codes as the device form (and FDGPU_EINVAL when first_id + n exceeds 32 bits or a varint is
 * malformed); the three arrays are released with fdgpu_free (out_offsets has n_hashes + 1 entries, out_hashes is a copy of hashes). */
int fdgpu_permute_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t n_hashes, const uint8_t *value, uint64_t value_len, uint64_t first_id,
                       const uint32_t *new_id, uint64_t n, uint32_t n_threads, uint8_t **out_value, uint64_t *out_value_len,
                       uint32_t **out_hashes, uint64_t **out_offsets);

/* Rows of the transposed index: for the structures id_lo .. id_hi - 1 (absolute ids, first_id <= id_lo <= id_hi <= first_id + n_structures)
 * (*row_off)[k] .. [k + 1] delimit, in *hashes, the ascending hashes whose posting lists hold structure id_lo + k.  id_hi - id_lo + 1 offsets,
 * row_off[0] = 0; id_lo == id_hi: one offset, no hash.  The shape of fdgpu_hash_batch's output, and for an index built over a batch its content:
 * the rows of the window equal fdgpu_hash_batch(sort_dedup = 1) of the same structures.  Byte-identical from run to run.  Release both with
 * fdgpu_free.  The index is not changed.  Workspace follows the window, not the index: 16 bytes per posting inside it, 8 per structure of it, 34
 * per list (csrc/k_rows.hip).  FDGPU_EINVAL for a window outside the index and for a damaged index (offsets that do not ascend inside the value
 * bytes, a varint that leaves its list, an id outside [first_id, first_id + n_structures)), found before a decoded id is used as an address or a
 * key; FDGPU_ERANGE for a list of 4 GiB or more or 2^32 or more postings inside the window; FDGPU_EHIP when the workspace does not fit.  On any
 * error both outputs are NULL.  Lists that hold nothing of the window (head at or above id_hi; last id below id_lo where the index carries last
 * ids) are not decoded beyond their head, so damage behind it goes unseen there: fdgpu_index_verify is the check of a whole index. */
int fdgpu_index_rows(fdgpu_ctx *ctx, const fdgpu_index *ix, uint64_t id_lo, uint64_t id_hi, uint32_t **hashes, uint64_t **row_off);
/* The same rows from host arrays (the payload of PREFIX.offset and PREFIX), n_threads host threads (0 = 1); the result does not depend on their
 * number.  No device.  Same arrays and same error codes as the device form for an index without last ids (and FDGPU_EINVAL when first_id +
 * n_structures exceeds 32 bits); both arrays are released with fdgpu_free. */
int fdgpu_rows_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t n_hashes, const uint8_t *value, uint64_t value_len,
                    uint64_t first_id, uint64_t n_structures, uint64_t id_lo, uint64_t id_hi, uint32_t n_threads,
                    uint32_t **row_hashes, uint64_t **row_off);

/* ---- index signatures --------------------------------------------------------------------------------------------------------
 * A fixed-size reduction of a structure's row R (the set of distinct hashes whose posting lists hold it; what fdgpu_index_rows returns).
 * With m(h) the splitmix64 finaliser of a hash, all arithmetic mod 2^64:
 *     z = (uint64)h + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  m = z ^ (z >> 31)
 * the signature holds |R|, the sum and the xor of m over R (equal rows give equal digests) and a one-permutation MinHash of 64 buckets: bucket
 * b = m >> 58 keeps the smallest v = (uint32_t)(m >> 26) of its hashes, 0xFFFFFFFF when it has none.  A v of 0xFFFFFFFF in a bucket that is not
 * empty reads as empty; every form (device, host, indexio.signatures_from_rows) does the same by construction.  An empty row: n = 0, d0 = d1 = 0,
 * every sk 0xFFFFFFFF.  The signature is a function of the row alone, so it moves with the structure under permute, rebase, split, merge and
 * remove.  280 bytes, little endian. */
typedef struct fd_signature {
    uint32_t n;               /* |R| */
    uint32_t reserved;        /* 0 */
    uint64_t d0;              /* sum of m(h) over R, mod 2^64 */
    uint64_t d1;              /* xor of m(h) over R */
    uint32_t sk[64];          /* bucket minima */
} fd_signature;
/* A reported pair of signatures a (of table A) and b (of table B), positions in their tables.  With E = buckets empty in both,
 * match = buckets that agree - E, filled = 64 - E: the pair is reported iff a.n > 0 && b.n > 0 && filled > 0 && match * 64 >= thr64 * filled
 * (integers only: the device and the host form agree exactly); match / filled estimates the Jaccard similarity of the two rows.
 * flags bit 0 (identical): n, d0 and d1 agree.  12 bytes. */
typedef struct fd_sig_pair { uint32_t a, b; uint8_t match, filled; uint16_t flags; } fd_sig_pair;
#define FD_SIG_IDENTICAL 1u

/* Signatures of the structures id_lo .. id_hi - 1 of a resident index (absolute ids, the range rule of fdgpu_index_rows): *out holds
 * id_hi - id_lo records, released with fdgpu_free.  The index is walked in windows of `window` structures (0 = 16384): per window the rows stay
 * on the device (the stages of fdgpu_index_rows without the copy out) and one wavefront per row reduces them (csrc/k_sig.hip); the result does
 * not depend on `window` and is byte-identical from run to run.  Workspace follows the window as for the rows, plus 280 bytes per structure of
 * it.  The refusals and error codes are those of fdgpu_index_rows, with the message prefix "index signatures:"; on any error *out is NULL. */
int fdgpu_index_signatures(fdgpu_ctx *ctx, const fdgpu_index *ix, uint64_t id_lo, uint64_t id_hi, uint64_t window, fd_signature **out);
/* The same signatures from host arrays (the payload of PREFIX.offset and PREFIX) by another algorithm: one pass over the lists, m(h) once per
 * list, every decoded id of the range updates its record.  n_threads host threads (0 = 1); the result does not depend on their number.  No
 * device.  Same records and same error codes as the device form for an index without last ids (and FDGPU_EINVAL when first_id + n_structures
 * exceeds 32 bits); released with fdgpu_free. */
int fdgpu_signatures_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t n_hashes, const uint8_t *value, uint64_t value_len,
                          uint64_t first_id, uint64_t n_structures, uint64_t id_lo, uint64_t id_hi, uint32_t n_threads, fd_signature **out);
/* Every pair (a of A, b of B) that is reported at thr64 (1 .. 64), sorted ascending by (a, b): byte-identical from run to run.  A and B are
 * host tables; B == NULL is self mode: A against itself, only a < b reported (nB is ignored).  More than max_pairs qualifying pairs:
 * FDGPU_ERANGE, *n_pairs = the true count, *pairs NULL.  thr64 outside 1 .. 64 or nA / nB >= 2^32: FDGPU_EINVAL before any device work.
 * *pairs (never NULL on success) is released with fdgpu_free. */
int fdgpu_signature_pairs(fdgpu_ctx *ctx, const fd_signature *A, uint64_t nA, const fd_signature *B, uint64_t nB, uint32_t thr64,
                          uint64_t max_pairs, fd_sig_pair **pairs, uint64_t *n_pairs);
/* The same pairs on the CPU (a blocked double loop, n_threads host threads, 0 = 1).  No device. */
int fdgpu_signature_pairs_host(const fd_signature *A, uint64_t nA, const fd_signature *B, uint64_t nB, uint32_t thr64, uint64_t max_pairs,
                               uint32_t n_threads, fd_sig_pair **pairs, uint64_t *n_pairs);

/* ---- signature neighbours: for every signature q of a table Q its k nearest among the signatures d of a table D.
 * With eq, E, match = eq - E and filled = 64 - E as for fd_sig_pair:
 *   candidate  d is a candidate of q iff the pair would be reported at thr64 (q.n > 0 && d.n > 0 && filled > 0 && match * 64 >= thr64 * filled;
 *              thr64 = 1: at least one agreeing filled bucket) and d is not excluded for q.
 *   exclusion  exclude[nQ] (optional) names one position of D per query that is never its neighbour, 0xFFFFFFFF = none.  D == NULL is self
 *              mode: the candidates are Q itself, exclude[q] = q is implied and a passed array is refused.  Both directions are produced:
 *              every signature gets its own list.
 *   order      x is nearer to q than y iff match_x * filled_y > match_y * filled_x, or these are equal and filled_x > filled_y (more buckets of
 *              evidence), or those are equal too and id_x < id_y (csrc/fd_signature.h: fd_sig_nearer).  Integers only and a total order: the
 *              result is unique and does not depend on the order in which the candidates are met.  The identical flag does not enter the order.
 *   result     nQ x k records, row q = q's nearest candidates in that order; id is a position in D (in Q in self mode), flags bit 0
 *              FD_SIG_IDENTICAL as in fd_sig_pair.  A slot beyond q's number of candidates holds id = 0xFFFFFFFF and zeros elsewhere; a query
 *              with n == 0 has only such slots.  8 bytes. */
typedef struct fd_sig_neighbor { uint32_t id; uint8_t match, filled; uint16_t flags; } fd_sig_neighbor;
#define FD_SIG_MAX_K 32u
/* The neighbours on the device (csrc/k_sig.hip: k_sg_near, one query per lane with its k-list in LDS, k_sg_near_merge when the candidates were
 * split over several workgroups).  Q and D are host tables; *out holds max(nQ * k, 1) records, released with fdgpu_free, byte-identical from
 * run to run and for every split.  FDGPU_EINVAL with a message opening "signature neighbors:", before any device work and with *out NULL:
 * k outside 1 .. FD_SIG_MAX_K, thr64 outside 1 .. 64, a table of 2^32 or more signatures, exclude together with D == NULL, a NULL table with a
 * non-zero count.  nQ == 0: an empty result; nD == 0: rows of empty slots.  Workspace: 280 bytes per signature, 8 * k per query and per
 * split.  Test switch, read per call: FDGPU_SG_NB_SPLIT=n sets the number of splits (clamped to 1 .. min(tiles of 64 candidates, 64)). */
int fdgpu_signature_neighbors(fdgpu_ctx *ctx, const fd_signature *Q, uint64_t nQ, const fd_signature *D, uint64_t nD, const uint32_t *exclude,
                              uint32_t k, uint32_t thr64, fd_sig_neighbor **out);
/* The same neighbours on the CPU: blocks of 64 queries against blocks of 64 candidates, n_threads host threads over the query blocks (0 = 1),
 * every query inserting into its own k-list; the result does not depend on n_threads.  No device.  The same refusals (code only). */
int fdgpu_signature_neighbors_host(const fd_signature *Q, uint64_t nQ, const fd_signature *D, uint64_t nD, const uint32_t *exclude, uint32_t k,
                                   uint32_t thr64, uint32_t n_threads, fd_sig_neighbor **out);

/* ---- signature clusters: one representative per group of a table S, every member reported with its representative.
 * The result is a function of S[0 .. n), a walk order (a permutation of the positions 0 .. n - 1; NULL = position order) and thr64 alone.
 * The positions are visited as p = order[0], order[1], ...:
 *   S[p].n == 0   p is unclustered: its record is {id = 0xFFFFFFFF, 0, 0, 0}.  Never a representative, never a candidate.
 *   otherwise     the candidates of p are the representatives chosen so far whose pair with p would be reported at thr64 (eq, E, match and
 *                 filled as for fd_sig_pair).  No candidate: p becomes a representative, its record is {id = p, match = filled = the number
 *                 of its non-empty buckets, flags = FD_SIG_IDENTICAL}.  Otherwise p joins the nearest candidate r in the order of the
 *                 neighbours (the larger match / filled, then the larger filled, then the smaller position in the table, not in the walk):
 *                 its record is {id = r, match, filled, flags bit 0 = n, d0 and d1 agree}.
 * Integers only and a total order: the result is unique.  No two representatives are a reported pair at thr64, every member is one with its
 * representative.  One fd_sig_neighbor per position; *out holds max(n, 1) of them, released with fdgpu_free, byte-identical from run to run.
 * FDGPU_EINVAL and *out NULL: thr64 outside 1 .. 64, n >= 2^32, a NULL table with n > 0, an order that is not a permutation of 0 .. n - 1
 * (a repeat, or a value >= n).  n == 0: an empty result.
 * On the device (csrc/k_sig.hip) no pair list is made: the walk goes in blocks of 256 positions; k_sg_cl_scan compares a block with the
 * representatives chosen so far (a compact device table that is only appended to; its count stays on the device), k_sg_cl_resolve merges
 * the splits, settles the block in walk order and appends its new representatives.  Stream order alone orders the steps, the host waits
 * once at the end.  The message of a refusal opens "signature clusters:" and nothing is launched.  Workspace: 2 * 280 + 8 bytes per
 * signature, 2 KB per split.  Test switch, read per call: FDGPU_SG_CL_SPLIT=n sets the number of splits of the scan (clamped to
 * 1 .. min(tiles of 64 representatives there can be, 256)); the result does not depend on it. */
int fdgpu_signature_clusters(fdgpu_ctx *ctx, const fd_signature *S, uint64_t n, const uint32_t *order, uint32_t thr64, fd_sig_neighbor **out);
/* The same clusters on the CPU: the same walk in blocks, n_threads host threads (0 = 1) over a block's positions for the scan of the
 * representatives chosen before the block; the result does not depend on n_threads.  No device.  The same refusals (code only). */
int fdgpu_signature_clusters_host(const fd_signature *S, uint64_t n, const uint32_t *order, uint32_t thr64, uint32_t n_threads,
                                  fd_sig_neighbor **out);

/* ---- seeded clusters: the walk above with a seed table T[0 .. nT) whose representatives already stand ("which of S is new").
 *   seeds         every T[j] with T[j].n > 0 is a representative from the start, unconditionally: two seeds that are a reported pair both
 *                 stand.  A seed with n == 0 is never a candidate.
 *   candidates    of p: the seeds and the representatives chosen so far from S whose pair with p would be reported at thr64.
 *   order         fd_sig_nearer over a combined id space: seed j has id j, position p of S has id nT + p.  So on a full tie of match / filled
 *                 and filled a seed beats a representative of S (what is already there is kept); within one table the smaller position wins.
 *   record        {id, match, filled, flags}; flags bit 1, FD_SIG_SEED: id is a position in T, else in S.  A new representative stays
 *                 {p, k, k, FD_SIG_IDENTICAL}, an unclustered position {0xFFFFFFFF, 0, 0, 0}.  A member of a seed is never a candidate.
 * Integers only and a total order: the result is unique.  nT == 0 (T may be NULL), or seeds that all have n == 0: byte for byte the result
 * of fdgpu_signature_clusters.  FDGPU_EINVAL and *out NULL, before any device work, the message opening "signature clusters:": the refusals
 * of the unseeded call, T == NULL with nT > 0, nT + n > 0xFFFFFFFF (the combined ids leave 0xFFFFFFFF free).
 * On the device the seeds never enter the table of representatives.  They do not change during the walk, so k_sg_cl_seed finds every
 * position's nearest seed in ONE launch over all blocks (grid: blocks of 256 positions x splits of the seed tiles; k_sg_cl_seed_merge reduces
 * the splits' partial bests when there are several), and k_sg_cl_resolve starts each lane from it: the walk then scans only the
 * representatives S itself adds, whose records carry nT + p.  Workspace beyond the unseeded call's: 280 bytes per seed, 8 per position, and
 * 8 per position and split when split: the splits are min(tiles of 64 seeds, 256, ceil(4096 / blocks)), so at most 8 MiB + 8 * n bytes.
 * Test switch, read per call: FDGPU_SG_CL_SEED_SPLIT=n sets the splits (clamped to 1 .. min(tiles of 64 seeds, 256): at most 2 KB per
 * position); the result does not depend on it. */
#define FD_SIG_SEED 2u
int fdgpu_signature_clusters_seeded(fdgpu_ctx *ctx, const fd_signature *S, uint64_t n, const uint32_t *order, const fd_signature *T, uint64_t nT,
                                    uint32_t thr64, fd_sig_neighbor **out);
/* The same on the CPU: every position's nearest seed with n_threads host threads (0 = 1) over the positions, then the blocked walk of
 * fdgpu_signature_clusters_host; the result does not depend on n_threads.  No device.  The same refusals (code only). */
int fdgpu_signature_clusters_seeded_host(const fd_signature *S, uint64_t n, const uint32_t *order, const fd_signature *T, uint64_t nT, uint32_t thr64,
                                         uint32_t n_threads, fd_sig_neighbor **out);

/* ---- exact row overlaps ------------------------------------------------------------------------------------------------------
 * For structures a and b with rows R_a and R_b (the ascending distinct hashes whose posting lists hold them; what fdgpu_index_rows returns):
 * the overlap is the integer inter = |R_a ∩ R_b|, union = |R_a| + |R_b| - inter, jaccard = inter / max(union, 1).  Integers only: the device
 * form, the host form and a plain set intersection agree exactly.  A row set keeps the rows of chosen structures on the device; the
 * intersect takes pairs of its row slots. */
typedef struct fdgpu_rowset fdgpu_rowset;      /* rows of chosen structures, resident on the device */

/* ids[0 .. n_ids): absolute structure ids of ix, strictly ascending.  Rows are taken in that order, window by window (windows of `window`
 * structures, 0 = 16384, each starting at the first id not yet taken), until taking the next id's row would bring the set above max_hashes
 * hashes; the first row of a call is always taken, whatever its size (max_hashes == 0: no limit).  *n_taken = the number of ids whose rows
 * are in the set (a prefix of ids).  Row k of the set is the row of ids[k].
 * The budget depends on the lengths of the rows alone: with L_k = |row of ids[k]|, n_taken is the largest t with t <= 1 or
 * L_0 + .. + L_(t-1) <= max_hashes.  `window` decides which rows one pass over the index extracts, never which are taken.
 * Per window the device stage of fdgpu_index_rows runs as it is, then a gather copies only the wanted rows into a block of the set (one
 * block per window, from the allocator the indices share; lengths and destinations from a scan, no atomics); the full rows of a window
 * never leave the device (csrc/k_overlap.hip).  FDGPU_EINVAL with a message opening "index rowset:", before any launch, no stage recorded
 * and *out NULL: ids that do not ascend strictly, an id outside [first_id, first_id + n_structures), ids NULL with n_ids > 0, 2^32 or
 * more ids.  A damaged index gives the codes of fdgpu_index_rows.  n_ids == 0: an empty set.  On any error *out is NULL, no device block is
 * kept and the context stays usable.  Release with fdgpu_rowset_destroy. */
int fdgpu_index_rowset(fdgpu_ctx *ctx, const fdgpu_index *ix, const uint32_t *ids, uint64_t n_ids, uint64_t window, uint64_t max_hashes,
                       fdgpu_rowset **out, uint64_t *n_taken);
int fdgpu_rowset_info(const fdgpu_rowset *rs, uint64_t *n_rows, uint64_t *n_hashes);
/* lengths[k] = |row k|: max(n_rows, 1) values from the set's host side (no device work), released with fdgpu_free */
int fdgpu_rowset_lengths(const fdgpu_rowset *rs, uint32_t **lengths);
/* the set as CSR: hashes[row_off[k] .. row_off[k + 1]) = row k; n_rows + 1 offsets; both released with fdgpu_free */
int fdgpu_rowset_export(fdgpu_ctx *ctx, const fdgpu_rowset *rs, uint32_t **hashes, uint64_t **row_off);
/* inter[p] = |row ka[p] of A  ∩  row kb[p] of B| for p < n_pairs, in the order of the pairs; B == NULL: both rows from A.  max(n_pairs, 1)
 * values, released with fdgpu_free.  One wavefront per pair walks both rows in 64-element tiles; the pairs are handed out longest first and
 * the results written back in input order; a pure function of the two rows, no global atomic.  FDGPU_EINVAL with a message opening
 * "rowset intersect:", before any launch, no stage recorded and *inter NULL: ka or kb NULL with n_pairs > 0, a slot >= the set's row
 * count, 2^32 or more pairs.  n_pairs == 0: an empty result. */
int fdgpu_rowset_intersect(fdgpu_ctx *ctx, const fdgpu_rowset *A, const fdgpu_rowset *B, const uint32_t *ka, const uint32_t *kb,
                           uint64_t n_pairs, uint32_t **inter);
void fdgpu_rowset_destroy(fdgpu_rowset *rs);
/* the same intersect over host CSR arrays (rows ascending, as fdgpu_index_rows / fdgpu_rows_host return them; n_a and n_b are row counts,
 * off_b == NULL: both rows from A), n_threads host threads (0 = 1), result independent of their number; no device.  The same refusals
 * (code only; and FDGPU_EINVAL for offsets that descend); *inter is released with fdgpu_free. */
int fdgpu_rows_intersect_host(const uint32_t *ha, const uint64_t *off_a, uint64_t n_a, const uint32_t *hb, const uint64_t *off_b, uint64_t n_b,
                              const uint32_t *ka, const uint32_t *kb, uint64_t n_pairs, uint32_t n_threads, uint32_t **inter);

/* ---- exact neighbours: for every row of a row set Q its k nearest structures of a resident index D by the Jaccard similarity of the rows.
 * D holds the structures first_id .. first_id + S - 1; d_len[S] is the length of each one's row in D, supplied by the caller (the n of the
 * signatures).  For query q with row R_q and structure s:
 *   inter      the number of h in R_q whose posting list in D holds s: |R_q ∩ R_s|, counted by one walk over the lists of R_q's hashes; the
 *              rows of D are never made
 *   uni        |R_q| + d_len[s - first_id] - inter
 *   candidate  s is a candidate of q iff inter > 0, s != exclude[q] (optional array of absolute ids of D, 0xFFFFFFFF = none) and
 *              inter * 10^4 >= floor_e4 * uni in 64-bit integers (floor_e4 in 0 .. 10000; 0: any shared hash)
 *   order      x is nearer than y iff inter_x * uni_y > inter_y * uni_x (u64), or these are equal and inter_x > inter_y, or those are equal too
 *              and id_x < id_y (csrc/fd_row_neighbor.h).  Integers only and a total order: the result is unique and does not depend on the
 *              launch geometry or on the order in which the lists are walked
 *   result     nQ x k records, row q = q's nearest candidates in that order; id is the absolute id in D; flags bit 0, FD_ROW_EQUAL: inter ==
 *              |R_q| == d_len[s], the two rows are the same set.  A slot beyond q's number of candidates holds {0xFFFFFFFF, 0, 0, 0}; a query
 *              with an empty row has only such slots.  k is in 1 .. 32.  16 bytes. */
typedef struct fd_row_neighbor { uint32_t id, inter, uni, flags; } fd_row_neighbor;
#define FD_ROW_EQUAL 1u
/* The neighbours on the device (csrc/k_exact.hip).  The queries go in blocks of QB = clamp(max_counter_bytes / (4 * S), 1, nQ) rows
 * (max_counter_bytes == 0: 1 GiB), each block with a u32 counter table [QB][S] in a context workspace: k_xn_count (one wavefront per 64
 * hashes of a query row: a binary search per lane in D's hash table, then the 64 lists walked in turn, one no-return atomic add per decoded
 * id) and k_xn_select (grid: query x split of the id range; every lane keeps a k-list in LDS, the wavefront merges them; k_xn_merge reduces
 * the splits when there are several).  Integer adds commute: the table, and with it the result, is byte-identical from run to run and for
 * every split and counter budget.  *out holds max(nQ * k, 1) records, released with fdgpu_free.
 * FDGPU_EINVAL with a message opening "rowset neighbors:", before any launch, no stage recorded and *out NULL: Q or D NULL, k outside
 * 1 .. 32, floor_e4 > 10000, d_len NULL with S > 0, an exclude id that is neither 0xFFFFFFFF nor inside D, a row set of another context.
 * nQ == 0: an empty result.  Behind the kernels, FDGPU_EINVAL and *out NULL, the context still usable: a counter above min(|R_q|, d_len)
 * ("row lengths do not belong to this index"), or a damaged index (offsets that do not ascend inside the value bytes, a varint that leaves
 * its list, an id outside D — such an id raises the flag and is never used as an address).
 * Test switch, read per call: FDGPU_XN_SPLIT=n sets the splits of the selection (clamped to 1 .. min(tiles of 64 ids, 64)); the result
 * does not depend on it.  Workspace: 4 * QB * S bytes of counters, 4 * S + 4 * nQ, 8 per 64 hashes of Q, 16 * k per query and per split. */
int fdgpu_rowset_neighbors(fdgpu_ctx *ctx, const fdgpu_rowset *Q, const fdgpu_index *D, const uint32_t *d_len, const uint32_t *exclude, uint32_t k,
                           uint32_t floor_e4, uint64_t max_counter_bytes, fd_row_neighbor **out);
/* The same neighbours over host arrays: the query rows as CSR (ascending distinct hashes, as fdgpu_index_rows returns them) and the files of
 * D.  n_threads host threads (0 = 1) over ranges of queries, each with one counter array of S that it resets where it touched it; the
 * result does not depend on their number.  No device.  The same records and the same refusals (code only; and FDGPU_EINVAL for query
 * offsets that descend or first_id + S above 0xFFFFFFFF). */
int fdgpu_rows_neighbors_host(const uint32_t *q_hashes, const uint64_t *q_off, uint64_t nQ, const uint32_t *d_hashes, const uint64_t *d_offsets,
                              uint64_t n_hashes, const uint8_t *d_value, uint64_t value_len, uint64_t first_id, uint64_t S, const uint32_t *d_len,
                              const uint32_t *exclude, uint32_t k, uint32_t floor_e4, uint32_t n_threads, fd_row_neighbor **out);

/* ---- index verification -----------------------------------------------------------------------------------------------------
 * Is an index well formed?  The definition (eight classes of damage, three on the hashes / offsets table and five on the posting
 * lists) is csrc/fd_verify.h and DESIGN.md; nothing else in the library checks the bytes it is given, every kernel uses offsets and
 * decoded ids as addresses.  A slot is a position 0 .. n_hashes of the offsets table; class c is bit (c - 1) of a slot's mask.
 * Every field is a pure function of the index: the device and the host checker fill the same report, bit for bit. */
#define FD_VERIFY_OFFSET_ENDS 1
#define FD_VERIFY_OFFSET_ORDER 2
#define FD_VERIFY_HASH_ORDER 3
#define FD_VERIFY_LIST_END 4
#define FD_VERIFY_VARINT_LONG 5
#define FD_VERIFY_VARINT_FORM 6
#define FD_VERIFY_ZERO_DELTA 7
#define FD_VERIFY_ID_RANGE 8
typedef struct fd_verify_report {
    uint32_t ok;              /* 1: no slot shows any class */
    uint32_t first_mask;      /* classes of the lowest bad slot */
    uint64_t n_bad;           /* slots that show at least one class */
    uint64_t class_count[9];  /* [c]: slots that show class c (1..8); [0] unused */
    uint64_t first_slot;      /* the lowest bad slot, its offsets[] entry and its hash (0 for slot n_hashes); all 0 when ok */
    uint64_t first_offset;
    uint32_t first_hash;
    uint32_t list_stage;      /* 1: the table was clean and the lists were decoded */
    uint64_t n_lists, n_postings, max_id, max_list_bytes;      /* of a clean index (ok == 1), else 0 */
} fd_verify_report;
/* Checks a resident index (built, merged, pruned, sliced or loaded; ids first_id .. first_id + n_structures - 1) on the device: a table
 * kernel, then - only if it found nothing - one decode pass over every value byte.  Returns FDGPU_OK when the check ran, whatever the
 * verdict.  The list pass reads nothing outside the value bytes + their slack, whatever they hold. */
int fdgpu_index_verify(fdgpu_ctx *ctx, const fdgpu_index *index, fd_verify_report *report);
/* The same check on host arrays (the payload of PREFIX.offset and PREFIX), n_threads host threads over slot ranges (0 = 1).  No device. */
int fdgpu_verify_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t n_hashes, const uint8_t *value, uint64_t value_len,
                      uint64_t first_id, uint64_t n_structures, uint32_t n_threads, fd_verify_report *report);

/* `analyze -p`: right-tail hypergeometric test of every encoding (src/controller/summary.rs:543-628, get_enriched_hashes /
 * hypergeometric_test with the reference's log-factorial): p_value[k] = P(X >= query_count[k]) for a sample of total_query draws from a
 * population of total_bg + total_query holding bg_count[k] + query_count[k] successes.  Host threads; no device needed. */
int fdgpu_hypergeom_enrichment(const uint64_t *query_count, const uint64_t *bg_count, uint64_t n_encodings, uint64_t total_query, uint64_t total_bg,
                               uint32_t n_threads, double *p_value);

/* Pairs that the speculative torsion evaluation of the index build (fd_geom.h, fd_pair_both_spec) re-evaluated with the
 * exact routine since the previous call; FDGPU_EXACT=1 in the environment disables the speculative path altogether. */
int fdgpu_spec_fallbacks(fdgpu_ctx *ctx, uint64_t *out);

/* ---- profiling hooks ------------------------------------------------------------------------------
 * Per-kernel timing of the last fdgpu_index_build / fdgpu_count_query call, measured with
 * HIP events on the context's stream. names[i] is a static string. Returns the number of
 * entries written (<= cap).  Every count call, fdgpu_count_query included, reports its scoring as
 * "cq_batch" and a device selection as "cq_topn". */
int fdgpu_last_timings(const fdgpu_ctx *ctx, const char **names, float *ms, uint64_t *bytes, int cap);
int fdgpu_enable_timing(fdgpu_ctx *ctx, int on);

/* ---- PREFIX.lookup (src/index/lookup.rs:35-56; written by build_index.rs:204-215) -------------------------------------------------
 * One line per structure: id \t tid \t nres \t plddt \t db_key \n, plddt printed like Rust's `{}` of an f32 (shortest digits that
 * round-trip, never exponent form, integral values without a fraction, NaN / inf spelled so).  tids = the n ids joined by '\n';
 * db_keys NULL = the id.  fdgpu_format_f32_display writes the n strings NUL-terminated at out + 64 * k. */
int fdgpu_write_lookup(const char *path, const char *tids, uint64_t n, const uint64_t *nres, const float *plddt, const uint64_t *db_keys);
int fdgpu_format_f32_display(const float *v, uint64_t n, char *out);

#ifdef __cplusplus
}
#endif
#endif
