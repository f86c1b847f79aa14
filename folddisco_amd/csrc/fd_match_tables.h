// fd_match_tables.h — the host block of a pair scan (fd_match_tables.cpp): what fd_match_pairs_multi computes on the host before its first launch.
//   work items     (query, candidate slot, 64-residue i-tile, span of partner residues): their number and span, and either every candidate's first
//                  item and query (k_mp_items writes the items on the device) or the four item arrays
//   query tables   per query mp_query_dev, its hashes, its observed distances grouped by (aa_i, aa_j) behind a 1,025-entry start table
//   intervals      queries of more than 1,024 observed distances: per group the merged float intervals that pass the window test
//   layout, block  where each of these sits in the one block that goes to the device, and the block itself
// No device and no HIP call: the file builds with a plain host compiler.  fd_api_match.hip chooses the buffer and uploads it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/fdgpu.h"
#include "fd_host_pool.h"

// query hashes a drain copies into LDS; fdgpu_internal.h defines it for the kernels (and the tests read it there).  Restated here, token for token, for a
// build of this header alone: the preprocessor reports a redefinition that differs
#define MP_QH_LDS 1024
struct mp_query_dev {   // per-query table of the pair scan (many queries in one launch)
    uint32_t qh_off, n_hashes;   // sorted unique hashes: q_hashes[qh_off .. +n_hashes)
    uint32_t aad_off, n_aad;     // grouped aa_dist_map: aad_dist / aad_qi [aad_off .. +n_aad); start table aad_start[1025 * query]
    uint32_t aa1_mask, aa2_mask; // residue types of the hashes' first / second residue (prefilter_amino_acid)
    int use_prefilter;
    float ca_window;
    uint32_t qs_off, qs_mask;    // more than MP_QH_LDS hashes: an open-addressing set of them, qset[qs_off .. + qs_mask + 1) (0xffffffff = empty); qs_mask = 0: none
};

// Word offsets of the block's sections, in block order; every section starts on a multiple of four words (16 bytes).  wc .. wj hold n_work words each,
// written by the host or (device-written items) by k_mp_items from wbase / cq, which exist only then; the three iv sections only with intervals.
struct mp_layout {
    size_t cand = 0, wc = 0, wi = 0, wq = 0, wj = 0, hashes = 0, start = 0, dist = 0, qi = 0, qtab = 0, iv_start = 0, iv = 0, iv_grp = 0, wbase = 0, cq = 0, words = 0;
};
inline size_t mp_up4(size_t n) { return (n + 3) & ~(size_t)3; }

// a scan's queries and candidates as the table builder reads them: query t scans cand[cand_off[t] .. cand_off[t + 1]); res_off: the batch's host offsets
struct mp_tables_in {
    uint64_t n_queries; const fd_match_query *qs; const uint32_t *cand; const uint64_t *cand_off; const uint64_t *res_off; uint64_t n_struct;
    uint32_t hash_type; bool dev_items;
};
struct mp_items {
    uint32_t j_span = 0; size_t n_wi = 0;
    std::vector<uint32_t> wbase, cq;              // device-written items: every candidate's first item (+ the total), its query
    std::vector<uint32_t> wc, wi, wq, wj;         // host-built items: candidate slot, first residue of the i-tile, query, first partner residue
};
struct mp_query_tabs {
    std::vector<mp_query_dev> qtab; std::vector<uint32_t> hashes, start, qi; std::vector<float> dist;
    uint64_t qset_slots = 0, qset_max_hashes = 0; bool want_iv = false;
};
struct mp_intervals { std::vector<uint32_t> iv_start; std::vector<float> lohi; };      // lohi: lo, hi interleaved (float2 on the device)
struct mp_built { mp_items W; mp_query_tabs T; mp_intervals V; };

// -> FDGPU_OK, or FDGPU_EINVAL / FDGPU_ERANGE with *err set (a candidate id outside the batch; 2^26 device-written items)
int mp_work_items(const mp_tables_in &in, mp_items &W, const char **err);
void mp_query_tables(const mp_tables_in &in, mp_query_tabs &T);
// pool: the helper threads for queries of 8,192 observed distances and more (null: serial); the result does not depend on it
void mp_interval_tables(uint64_t n_queries, const mp_query_tabs &T, fd_host_pool *pool, mp_intervals &V);
mp_layout mp_make_layout(uint64_t n_cand, uint64_t n_queries, bool dev_items, const mp_built &B);
// blk: L.words words of the caller's; the padding between sections is left as it is
void mp_pack(const mp_tables_in &in, const mp_layout &L, const mp_built &B, uint32_t *blk);

// host block of a pair scan's work items and query tables (fd_match_pairs_multi builds it on the first call, reuses it on the next)
struct fd_mp_tables {
    std::vector<uint32_t> blk; mp_layout L; size_t nw = 0; bool want_iv = false; uint32_t j_span = 0; bool valid = false;
    const uint32_t *data = nullptr;                         // the packed block: blk, or (tables not kept by the caller) the context's pinned staging buffer
    bool dev_items = false;                                 // work items written on the device from [first item | query] per candidate (one-off blocks)
    uint64_t qset_slots = 0, qset_max_hashes = 0;           // slots of the large queries' hash sets (mp_query_dev.qs_off / qs_mask), their largest hash count
};
// the three table steps and the layout: B for mp_pack, TB's scalars and layout set (TB.data / TB.valid are the caller's, once the block is packed)
int mp_build_tables(const mp_tables_in &in, fd_host_pool *pool, mp_built &B, fd_mp_tables &TB, const char **err);
