// fd_query_map_host.h — the host part of make_query_map (fd_query_map_host.cpp): what fdgpu_make_query_map_batch computes on the host around its kernels.
//   pairs            all ordered pairs of every query's residues, row-major (CombinationIterator, utils/combination.rs:23-44)
//   fields           the container fields an encoding's thresholds shift (controller/feature.rs:269-291)
//   observed lists   (aa_i, aa_j, CA distance, query residue) of the valid pairs within 20 A (structure/core.rs:462-477)
//   expansion        the host form of expand_and_insert with substitutions (query.rs:86-206): the candidates' containers in insertion order
//   first insertions first insertion wins over one query's insertions (the reference's hash map keeps the entry a hash was first inserted with)
//   arena, fill      where the arrays of one fd_query_map sit in its single block, and the block itself
// No device and no HIP call: the file builds with a plain host compiler — with the library's flags (-ffp-contract=off), which the expansion's
// single f32 adds need.  fd_query_map.hip runs the kernels between these steps.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <functional>
#include <vector>
#include "../../include/fdgpu.h"
#include "fd_host_pool.h"

// floats per pair / candidate in the query map's own record: [0..9) the feature container of get_single_feature, [9] the CA distance,
// [10], [11] the two residue types (k_pair_features12 writes it)
#define FD_QF 12

// from this many pairs / entries on, a loop over them runs in eight parts on the pool
#define QM_PARTS_MIN 16384
// n parts of a loop on `threads` threads of the pool (the caller among them; pool null or threads <= 1: inline, in part order).
// part(z) for every z in [0, n), each once.  Which part runs where does not show in any result here: parts write disjoint ranges.
void qm_run_parts(fd_host_pool *pool, unsigned threads, unsigned n, const std::function<void(unsigned)> &part);

// ---- pairs
struct qm_pairs { std::vector<uint32_t> pi, pj; std::vector<uint64_t> off; };      // residue indices of the whole batch; query t: [off[t], off[t + 1])
// query t = structure q_struct[t] (residues res_off[s] .. res_off[s + 1]) with the residues q_index[q_off[t] .. q_off[t + 1]): indices outside
// the structure are skipped, and so is the pair of a position with itself (a repeated residue still pairs with its other copies' partners)
void qm_list_pairs(uint64_t n_queries, const uint32_t *q_struct, const uint64_t *q_off, const uint32_t *q_index, const uint64_t *res_off, qm_pairs &P);

// ---- fields
struct qm_fields { int di[2], ndi, ai[7], nai; bool has_aa; };      // dist_index / angle_index; has_aa: fields 0, 1 are residue types (substitutions apply)
qm_fields qm_fields_of(uint32_t hash_type);

// ---- observed lists
struct qm_aad { std::vector<uint8_t> a1, a2; std::vector<float> ad; std::vector<uint32_t> aq; };
struct qm_feat { const float *feat; const uint8_t *valid; };      // [np][FD_QF], [np]
// pairs [k0, k1) of one query whose structure starts at residue r0; threads > 1: eight parts on the pool, joined in pair order
void qm_observed_list(const qm_feat &F, const uint32_t *pi, uint64_t k0, uint64_t k1, uint64_t r0, fd_host_pool *pool, unsigned threads, qm_aad &A);

// ---- expansion (host form)
struct qm_cand { uint32_t qi, qj; uint8_t primary; uint32_t pair; };
struct qm_cands { std::vector<float> vf; std::vector<qm_cand> c; };      // FD_QF floats per candidate
struct qm_thresholds { const float *dist; uint64_t n_dist; const float *angle_rad; uint64_t n_angle; };
// candidates of the valid pairs [k0, k1) of one query, appended in the reference's insertion order: the observed container; substitutions on i,
// i x j, or j (subs / n_subs run parallel to qidx[0 .. n_q), null = none; a later entry for the same residue overrides); then near / far per
// threshold and field, restored with f32 += / -= like the reference (not an exact inverse: the drift stays)
void qm_expand_query(const qm_feat &F, const uint32_t *pi, const uint32_t *pj, uint64_t k0, uint64_t k1, uint64_t r0, const uint32_t *qidx, uint64_t n_q,
                     const uint8_t *const *subs, const uint32_t *n_subs, const qm_fields &fl, const qm_thresholds &T, qm_cands &C);

// ---- first insertions
// insertion pos of a query = candidate c0 + pos / n_planes under bin configuration pos % n_planes: its hash is planes[pos % n_planes][c0 + pos / n_planes]
struct qm_insertions { const uint32_t *const *planes; uint32_t n_planes; uint64_t c0, n_ins; };
inline uint32_t qm_hash_at(const qm_insertions &I, uint64_t pos) { return I.planes[pos % I.n_planes][I.c0 + pos / I.n_planes]; }
#define QM_FI_TABLE_MAX 4096ull           // up to here an open-addressing table; above, (hash << 32 | position) keys through an LSD radix sort
#define QM_FI_SET_MIN (1ull << 32)        // from here (positions no longer fit a key's low word) a hash set
// keep: the positions that enter the map, ascending.  tab: scratch of the table form, reused from query to query
void qm_first_wins(const qm_insertions &I, std::vector<uint64_t> &tab, std::vector<uint32_t> &keep, uint64_t table_max = QM_FI_TABLE_MAX,
                         uint64_t set_min = QM_FI_SET_MIN);

// ---- arena and fill
// byte offsets of the arrays behind the fd_query_map at the head of its block, in block order; every one on a multiple of 16.  pl / pk / ps
// (posting length, list position, segments) take room only with_post.
struct qm_arena { size_t hash, qi, qj, idf, ph, pl, pk, ps, idx, ad, aq, prim, a1, a2, bytes; };
qm_arena qm_arena_layout(size_t n, size_t n_idx, size_t n_aad, bool with_post);

struct qm_map_src {      // what one query's map is filled from
    const uint32_t *keep; size_t n;                     // kept insertion positions, ascending
    qm_insertions ins;                                  // the query's insertions (hash of a position)
    const qm_cand *cands;                               // host form: candidate z -> (residues, observed?, pair); null = device forms, where
    const uint32_t *vpairs; uint64_t per_pair;          //   candidate z is insertion z % per_pair of valid pair vpairs[z / per_pair]
    const uint32_t *pi, *pj; uint64_t r0;
    const float *pair_idf; const uint32_t *pair_primary;      // per pair: idf and hash of its observed candidate
    const uint64_t *post_len; const uint32_t *post_seg; const long long *post_kidx; uint64_t index_uid;      // of the kept entries, or all null
    const uint32_t *indices; size_t n_idx;
    const qm_aad *aad;
};
// the map and all its arrays in ONE malloc'd block (arena_bytes != 0: fdgpu_query_map_free releases it); null = out of memory.  threads > 1: the
// device forms' entries in eight parts on the pool
fd_query_map *qm_fill_map(const qm_map_src &S, fd_host_pool *pool, unsigned threads);
