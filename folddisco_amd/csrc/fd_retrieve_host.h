// fd_retrieve_host.h — the retrieval's host glue (fd_retrieve_host.cpp): what a retrieval computes on host threads between its GPU stages.
//   per call    query tables (fd_rb_prepare), hash -> entry tables and sorted observed-distance lists of large queries
//   per slot    graph (src/controller/graph.rs:16-50) -> components -> votes -> assignment (retrieve.rs:604-702) -> rescue (:479-515) -> residue
//               lists -> records and Kabsch problems (fd_rh_slot), one candidate slot per call, every slot touched by one thread
//   per pass    the slots' outputs merged in slot order (fd_rh_merge_plan, fd_rh_merge_full)
// No device and no HIP call: the file builds with a plain host compiler.  fd_host_query.hip fills fd_rh_call and runs the slots on the context's pool.
#pragma once
#include <stdint.h>
#include <chrono>
#include <unordered_map>
#include <vector>
#include "../../include/fdgpu.h"

struct fd_vote_row { uint32_t mx, nmx, arg; };      // a row of the device-counted rescue votes (fd_vote_plan, fdgpu_internal.h)

// symmetry flag of a hash (geometry/pdb_tr.rs:158-162 and the other encodings' is_symmetric)
bool fd_hash_is_sym(uint32_t htype, uint32_t h);

struct fd_rh_graph {
    std::vector<uint32_t> w;           // node -> residue index (first-appearance order, graph.rs:16-26)
    std::vector<uint32_t> es, et, eh;  // edges in insertion order
    std::unordered_map<uint32_t, uint32_t> at;
    std::vector<int32_t> dense;        // residue -> node for residues below dense.size() (a candidate's residue count is known: no hashing
                                       // for the 6 x 10^4 lookups of a whole-structure query's heaviest candidate)
    uint32_t node_of(uint32_t res) {
        if (res < dense.size()) {
            int32_t &n = dense[res];
            if (n < 0) { n = (int32_t)w.size(); w.push_back(res); }
            return (uint32_t)n;
        }
        auto ins = at.emplace(res, (uint32_t)w.size());
        if (ins.second) w.push_back(res);
        return ins.first->second;
    }
};
// SCCs and weakly connected components of at least min_nodes nodes, as sorted node lists, sorted and without duplicates (graph.rs:29-50)
std::vector<std::vector<uint32_t>> fd_rh_components(const fd_rh_graph &g, size_t min_nodes);

// What a retrieval needs from the query maps alone — no candidates, no scan output: per query the sorted unique hashes + the map entry each one
// resolves to (the FIRST entry holding it, like the reference's hash map), the pair scan's query descriptors, sizes.  A caller that knows the
// maps before it knows the candidates (fdgpu_query_batch: the scoring kernels are still running) builds it ahead of time.
struct fd_rb_prep {
    std::vector<std::vector<uint32_t>> qhs, qkf;
    std::vector<fd_match_query> mqs;
    std::vector<uint32_t> q_sizes;
    uint64_t max_aad = 0, max_nq = 0;
};
void fd_rb_prepare(uint64_t n_queries, const fd_query_map *const *qms, float ca_distance_cutoff, fd_rb_prep &P);

// large queries (> 4096 hashes): hash -> map entry through an open-addressing table built once per query; e_tab[t] empty = bisection in qhs[t]
struct fd_rh_entry_tabs {
    std::vector<std::vector<uint64_t>> e_tab; std::vector<uint32_t> e_mask;
    explicit fd_rh_entry_tabs(uint64_t n_queries) : e_tab(n_queries), e_mask(n_queries ? n_queries : 1, 0) {}
};
void fd_rh_build_e_tab(const fd_rb_prep &P, fd_rh_entry_tabs &T);
// every query's observed-distance lists in the pair scan's group layout, every group sorted by distance (the second scan's vote loop, k_match.hip)
void fd_rh_build_sorted_lists(uint64_t n_queries, const fd_query_map *const *qms, std::vector<float> &sd_dist, std::vector<uint32_t> &sd_qi);

// two-scan retrievals build the components and from-hash mappings once (plan pass) and reuse them in the full pass
struct fd_rh_comp_plan { std::vector<uint32_t> q_idx, r_idx; float sub_idf = 0.0f; uint32_t rc_ord = 0; };      // rc_ord: 1-based ordinal among the slot's components that need the rescue
struct fd_rh_slot_plan { std::vector<fd_rh_comp_plan> comps; bool have = false; };
struct fd_rh_pend { size_t rec; int which; };      // a Kabsch problem's record; which: 0 from_hash, 1 processed
// Candidate slots are independent (their own found triples, candidate pairs and outputs): they are processed by a pool of
// host threads into per-slot outputs that are merged in slot order afterwards, so the result does not depend on the thread count.
struct fd_rh_slot_out {
    std::vector<fd_match_rec> recs; std::vector<int32_t> res;      // res: 2 * NQ per match, from_hash then processed target residue index (-1 = none)
    std::vector<float> kx, ky; std::vector<uint64_t> klen;         // Kabsch points (target = moving x, query = fixed y)
    std::vector<fd_rh_pend> pend; std::vector<uint32_t> marks, mark_ord;
};

// What every slot of one pass reads and none writes.  Arrays per slot hold n_cand (+ 1 where a range ends there) entries.
struct fd_rh_call {
    const fd_query_map *const *qms = nullptr; const fd_rb_prep *prep = nullptr; const fd_rh_entry_tabs *tabs = nullptr;
    const uint64_t *cand_off = nullptr; const uint32_t *slot_q = nullptr;      // slot -> query
    uint32_t hash_type = 0, node_count = 0;
    bool trace = false;
    std::chrono::steady_clock::time_point stage_t0;                              // for the trace lines of heavy slots
    // the scans' output, grouped by slot: found triples [f_lo[slot], f_lo[slot + 1]); candidate pairs [c_lo ...) either as records or packed
    // (key = slot << 16 | partner residue j, sorted; value = qi << 16 | i; fd_match_pairs_multi with MP_CANDS_PACKED)
    const fd_pair_rec *found = nullptr; const fd_cand_rec *cands = nullptr; const uint32_t *pk_key = nullptr, *pk_val = nullptr;
    const size_t *f_lo = nullptr, *c_lo = nullptr;
    // coordinates: the candidates' [CA of all | CB of all], slot k at residue g_dst[k]; the query structures' CA / CB, query t at residue q_res0[t]
    const float *t_all = nullptr; const uint64_t *g_dst = nullptr; uint64_t g_total = 0;
    const float *qb_ca = nullptr, *qb_cb = nullptr; const uint64_t *q_res0 = nullptr;
    // rescue votes counted by the second scan (null: counted here from the candidate pairs): rows of slot k from row_base[k], one per (ordinal, query residue)
    const fd_vote_row *vote_rows = nullptr; const uint64_t *row_base = nullptr;
};
// per-slot ranges of the found triples and candidate pairs (both arrive grouped by slot); f_lo, c_lo: n_cand + 1 entries
void fd_rh_slot_ranges(const fd_pair_rec *found, uint64_t nf, const fd_cand_rec *cands, const uint32_t *pk_key, uint64_t nc, uint64_t n_cand, size_t *f_lo, size_t *c_lo);
// One slot.  plan = true: components and mappings only, marking (o.marks / o.mark_ord) the mapped residues of every component that leaves a
// query residue unmatched (first pass of a large query); plan = false: the full body.  cache: the slot's plans in a two-scan call (written by the plan
// pass, read by the full pass), else null.
void fd_rh_slot(const fd_rh_call &C, uint64_t slot, bool plan, fd_rh_slot_plan *cache, fd_rh_slot_out &o);

// the plan pass's marks, in slot order -> the second scan's partner-residue filter (bit mask_off[slot] + residue) and, for votes counted on the
// device, per marked residue the ordinal of the component that mapped it
struct fd_rh_marks {
    std::vector<uint32_t> cj_mask; std::vector<uint8_t> cj_comp; std::vector<uint32_t> slot_nrc;      // slot_nrc: rescued components per slot
    bool any_rescue = false, vote_conflict = false;                                                     // vote_conflict: two rescued components share a target residue
};
void fd_rh_merge_plan(const std::vector<fd_rh_slot_out> &outs, const uint32_t *mask_off, fd_rh_marks &M);
// the full pass's records, residue lists and Kabsch problems in slot order; m_off / r_off: per query
struct fd_rh_merged {
    std::vector<fd_match_rec> recs; std::vector<int32_t> res; std::vector<float> kx, ky; std::vector<uint64_t> koff{0};
    std::vector<fd_rh_pend> pend; std::vector<uint64_t> m_off, r_off;
};
void fd_rh_merge_full(const std::vector<fd_rh_slot_out> &outs, uint64_t n_queries, const uint64_t *cand_off, fd_rh_merged &R);
