// fd_retrieve_host.cpp — the retrieval's host glue (fd_retrieve_host.h): query tables, and per candidate slot
//   graph -> components -> votes -> assignment -> rescue -> residue lists -> records + Kabsch problems
// (src/controller/retrieve.rs:364-552, graph.rs:16-50), then the merges of the slots' outputs.  No device and no HIP call: this file also builds
// with a plain host compiler (tools/check_retrieve_host.cpp runs it under the sanitizers).  It contains no f32 arithmetic that decides a hash bit.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <array>
#include "../../include/fdgpu_debug.h"
#include "fd_retrieve_host.h"

// the encodings' numbers (fd_hash_params.hash_type), as fd_geom.h and fd_geom_other.h define them for the device code
#define FD_HASH_TRROSETTA 2u
#define FD_HASH_PPF 4u
#define FD_HASH_TERTIARY 5u
#define FD_HASH_HYBRID 6u
#define FD_HASH_PDBMOTIF 0u
#define FD_HASH_PDBMOTIF_SINCOS 1u
#define FD_HASH_FD_ANGLE 7u
#define FD_HASH_FD_DIST 8u

namespace {
typedef std::chrono::steady_clock::time_point rh_time;
inline rh_time t_now() { return std::chrono::steady_clock::now(); }
inline double t_ms(rh_time a, rh_time b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
}  // namespace

// symmetry flags (geometry/pdb_tr.rs:158-162): aa equal and atan2(sin, cos) of the two torsion fields equal; the other encodings
// compare their residue fields and (Folddisco*) torsion fields (pdb_motif.rs:98, pdb_motif_sincos.rs:105, folddisco_angle.rs:133,
// folddisco_dist.rs:126)
bool fd_hash_is_sym(uint32_t htype, uint32_t h) {
    const float D2 = 57.2957795130823208767981548141051703f;
    auto c3 = [](uint32_t v, float nb) { float cf = (1.0f - (-1.0f)) / (nb - 1.0f); return (float)v * cf + (-1.0f); };
    if (htype == FD_HASH_TERTIARY) return false;                                   // tertiary_interaction.rs:145-150
    if (htype == FD_HASH_TRROSETTA) {                                              // trrosetta.rs:158-162 (default 3 angle bins)
        const uint32_t pr = (h >> 23) & 0x1ffu;
        float a[5];
        for (int k = 0; k < 5; ++k) a[k] = atan2f(c3((h >> (18 - 4 * k)) & 3u, 3.0f), c3((h >> (16 - 4 * k)) & 3u, 3.0f)) * D2;
        return pr / 20u == pr % 20u && a[1] == a[2] && a[3] == a[4];
    }
    if (htype == FD_HASH_PPF) {                                                    // ppf.rs:124-127
        float a[2];
        for (int k = 0; k < 2; ++k) a[k] = atan2f(c3((h >> (15 - 6 * k)) & 7u, 3.0f), c3((h >> (12 - 6 * k)) & 7u, 3.0f)) * D2;
        return ((h >> 27) & 31u) == ((h >> 22) & 31u) && a[0] == a[1];
    }
    if (htype == FD_HASH_HYBRID) {                                                 // hybrid.rs:185-189 (4 angle bins)
        float a[2];
        for (int k = 0; k < 2; ++k) a[k] = atan2f(c3((h >> (14 - 4 * k)) & 3u, 4.0f), c3((h >> (12 - 4 * k)) & 3u, 4.0f)) * D2;
        return ((h >> 30) & 3u) == ((h >> 28) & 3u) && a[0] == a[1];
    }
    if (htype == FD_HASH_PDBMOTIF) return ((h >> 20) & 31u) == ((h >> 15) & 31u);
    if (htype == FD_HASH_PDBMOTIF_SINCOS) return ((h >> 21) & 31u) == ((h >> 16) & 31u);
    if (htype == FD_HASH_FD_ANGLE || htype == FD_HASH_FD_DIST) {
        const uint32_t pair = (h >> 21) & 0x1ffu;
        const uint32_t p1 = htype == FD_HASH_FD_ANGLE ? (h >> 5) & 31u : (h >> 4) & 15u, p2 = htype == FD_HASH_FD_ANGLE ? h & 31u : h & 15u;
        return pair / 20u == pair % 20u && p1 == p2;
    }
    // the default encoding: the two torsion angles from their (sin, cos) bin pairs — sixteen possible pairs, atan2f of each evaluated once (the same
    // call on the same arguments: same floats); two atan2f per found edge were 0.8 ms of a whole-structure query's plan pass (25,162 edges of the self hit)
    static const std::array<float, 16> ang = [] {
        std::array<float, 16> t{};
        auto cont = [](uint32_t v) { float cf = (1.0f - (-1.0f)) / (4.0f - 1.0f); return (float)v * cf + (-1.0f); };
        const float D = 57.2957795130823208767981548141051703f;
        for (uint32_t v = 0; v < 16; ++v) t[v] = atan2f(cont(v >> 2), cont(v & 3u)) * D;
        return t;
    }();
    return ((h >> 25) & 31u) == ((h >> 20) & 31u) && ang[(h >> 4) & 15u] == ang[h & 15u];
}

// SCCs (Tarjan) and weakly connected components of at least min_nodes nodes, as sorted node lists, sorted and without duplicates (graph.rs:29-50).
// Flat arrays throughout: a 2,500-residue candidate of a whole-structure query has ~2,500 nodes, nearly all of them components of one node — a vector
// per node's neighbours and a map entry + a vector per component were 0.5 ms of such a slot
std::vector<std::vector<uint32_t>> fd_rh_components(const fd_rh_graph &g, size_t min_nodes) {
    const uint32_t n = (uint32_t)g.w.size();
    const size_t E = g.es.size();
    std::vector<uint32_t> a_off(n + 1, 0), a_to(E);
    for (size_t e = 0; e < E; ++e) ++a_off[g.es[e] + 1];
    for (uint32_t v = 0; v < n; ++v) a_off[v + 1] += a_off[v];
    {
        std::vector<uint32_t> cur(a_off.begin(), a_off.end() - 1);
        for (size_t e = 0; e < E; ++e) a_to[cur[g.es[e]]++] = g.et[e];       // a node's neighbours in edge order
    }
    std::vector<int> idx(n, -1), low(n, 0), comp(n, -1);
    std::vector<char> on(n, 0);
    std::vector<uint32_t> stk;
    int counter = 0, ncomp = 0;
    struct Fr { uint32_t v; uint32_t it; };
    std::vector<Fr> cs;
    for (uint32_t root = 0; root < n; ++root) {
        if (idx[root] >= 0) continue;
        cs.clear();
        cs.push_back({root, a_off[root]});
        idx[root] = low[root] = counter++; stk.push_back(root); on[root] = 1;
        while (!cs.empty()) {
            Fr &f = cs.back();
            if (f.it < a_off[f.v + 1]) {
                uint32_t x = a_to[f.it++];
                if (idx[x] < 0) { idx[x] = low[x] = counter++; stk.push_back(x); on[x] = 1; cs.push_back({x, a_off[x]}); }
                else if (on[x]) low[f.v] = std::min(low[f.v], idx[x]);
            } else {
                uint32_t v = f.v;
                if (low[v] == idx[v]) {
                    uint32_t x;
                    do { x = stk.back(); stk.pop_back(); on[x] = 0; comp[x] = ncomp; } while (x != v);
                    ++ncomp;
                }
                cs.pop_back();
                if (!cs.empty()) low[cs.back().v] = std::min(low[cs.back().v], low[v]);
            }
        }
    }
    std::vector<uint32_t> uf(n);
    for (uint32_t v = 0; v < n; ++v) uf[v] = v;
    auto find = [&uf](uint32_t x) { while (uf[x] != x) { uf[x] = uf[uf[x]]; x = uf[x]; } return x; };
    for (size_t e = 0; e < E; ++e) { uint32_t a = find(g.es[e]), b = find(g.et[e]); if (a != b) uf[a] = b; }
    // the sets of at least min_nodes nodes, their nodes ascending (a walk over the nodes in order); the result is the SORTED list of sets without
    // duplicates, so the order they are gathered in does not matter
    std::vector<std::vector<uint32_t>> all;
    auto gather = [&all, n, min_nodes](const std::vector<uint32_t> &label, uint32_t n_labels) {
        std::vector<uint32_t> size(n_labels, 0), at(n_labels, 0xffffffffu);
        for (uint32_t v = 0; v < n; ++v) ++size[label[v]];
        for (uint32_t v = 0; v < n; ++v) {
            const uint32_t l = label[v];
            if (size[l] < min_nodes || size[l] == 0) continue;
            if (at[l] == 0xffffffffu) { at[l] = (uint32_t)all.size(); all.emplace_back(); all.back().reserve(size[l]); }
            all[at[l]].push_back(v);
        }
    };
    std::vector<uint32_t> label(n);
    for (uint32_t v = 0; v < n; ++v) label[v] = (uint32_t)comp[v];
    gather(label, (uint32_t)ncomp);
    for (uint32_t v = 0; v < n; ++v) label[v] = find(v);
    gather(label, n);
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    return all;
}

void fd_rb_prepare(uint64_t n_queries, const fd_query_map *const *qms, float ca_distance_cutoff, fd_rb_prep &P) {
    std::vector<std::vector<uint32_t>> &qhs = P.qhs, &qkf = P.qkf;
    std::vector<fd_match_query> &mqs = P.mqs;
    std::vector<uint32_t> &q_sizes = P.q_sizes;
    qhs.assign(n_queries, {}); qkf.assign(n_queries, {});
    mqs.assign(std::max<uint64_t>(n_queries, 1), fd_match_query{});
    q_sizes.assign(std::max<uint64_t>(n_queries, 1), 1);
    P.max_aad = 0; P.max_nq = 0;
    // per query: sorted unique hashes + the map entry each one resolves to (the FIRST entry holding it, like the reference's hash map):
    // (hash << 32 | entry) keys through an LSD radix sort — a whole-structure query has 10^5 entries, a hash map cost 8 ms here
    for (uint64_t t = 0; t < n_queries; ++t) {
        const fd_query_map *m = qms[t];
        uint64_t key_small[256];          // a motif query's few dozen entries stay off the heap (two allocations per query, 128 queries per batch)
        std::vector<uint64_t> key_v, tmp_v;
        if (m->n > 256) { key_v.resize(m->n); tmp_v.resize(m->n); }
        uint64_t *key = m->n > 256 ? key_v.data() : key_small, *tmp = tmp_v.data();
        for (uint64_t k = 0; k < m->n; ++k) {
            key[k] = ((uint64_t)m->hash[k] << 32) | (uint32_t)k;
            q_sizes[t] = std::max(q_sizes[t], std::max(m->qi[k], m->qj[k]) + 1);
        }
        // the rescue (retrieve.rs:479-515) looks a residue of `indices` up in the candidate pairs whether or not a map entry names it: the tables indexed by
        // query residue cover those residues too (a residue all of whose pairs lie beyond the cutoff, or a hand-made map)
        for (uint64_t k = 0; k < m->n_indices; ++k) q_sizes[t] = std::max(q_sizes[t], (uint32_t)std::min<uint64_t>((uint64_t)m->indices[k] + 1, 0xffffffffull));
        if (m->n > 256) {
            for (int pass = 0; pass < 4; ++pass) {           // entries arrive in ascending k: a stable sort by hash keeps the first entry first
                const int sh = 32 + 8 * pass;
                size_t cnt[257] = {0};
                for (uint64_t k = 0; k < m->n; ++k) ++cnt[((key[k] >> sh) & 255u) + 1];
                for (int d = 0; d < 256; ++d) cnt[d + 1] += cnt[d];
                for (uint64_t k = 0; k < m->n; ++k) tmp[cnt[(key[k] >> sh) & 255u]++] = key[k];
                std::swap(key, tmp);
            }
        } else std::sort(key, key + m->n);
        qhs[t].reserve(m->n); qkf[t].reserve(m->n);
        for (uint64_t k = 0; k < m->n; ++k)
            if (k == 0 || (key[k] >> 32) != (key[k - 1] >> 32)) { qhs[t].push_back((uint32_t)(key[k] >> 32)); qkf[t].push_back((uint32_t)key[k]); }
        fd_match_query &q = mqs[t];
        q.hashes = qhs[t].data(); q.n_hashes = qhs[t].size();
        q.aad_aa1 = m->aad_aa1; q.aad_aa2 = m->aad_aa2; q.aad_dist = m->aad_dist; q.aad_qi = m->aad_qi; q.n_aad = m->n_aad;
        q.ca_distance_cutoff = ca_distance_cutoff;
        q.use_aa_prefilter = qhs[t].size() <= 200 ? 1 : 0;  // PREFILTER_AA_SKIPPING_SIZE (retrieve.rs:24, 569)
        P.max_aad = std::max<uint64_t>(P.max_aad, m->n_aad); P.max_nq = std::max<uint64_t>(P.max_nq, m->n_indices);
    }
}

// large queries: hash -> map entry through an open-addressing table built once per query (a whole-structure query looks ~10^5 found
// edges up in ~10^5 hashes per call: 17 bisection steps each were a quarter of the largest candidate's time)
void fd_rh_build_e_tab(const fd_rb_prep &P, fd_rh_entry_tabs &T) {
    const uint64_t n_queries = P.qhs.size();
    for (uint64_t t = 0; t < n_queries; ++t) {
        const std::vector<uint32_t> &qh = P.qhs[t], &qk = P.qkf[t];
        if (qh.size() <= 4096) continue;
        uint32_t cap = 1;
        while (cap < 2 * qh.size()) cap <<= 1;
        T.e_tab[t].assign(cap, ~0ull);
        T.e_mask[t] = cap - 1;
        for (size_t z = 0; z < qh.size(); ++z) {
            uint32_t at = (qh[z] * 2654435761u) & T.e_mask[t];
            while (T.e_tab[t][at] != ~0ull) at = (at + 1) & T.e_mask[t];
            T.e_tab[t][at] = ((uint64_t)qh[z] << 32) | qk[z];
        }
    }
}

// every query's observed-distance lists in the pair scan's group layout (counting sort by aa_i * 32 + aa_j, entries with
// residue types below 32, queries concatenated), every group sorted by distance — what the second scan's vote loop searches (k_match.hip)
void fd_rh_build_sorted_lists(uint64_t n_queries, const fd_query_map *const *qms, std::vector<float> &sd_dist, std::vector<uint32_t> &sd_qi) {
    std::vector<std::pair<float, uint32_t>> grp;
    for (uint64_t t = 0; t < n_queries; ++t) {
        const fd_query_map *m = qms[t];
        std::vector<uint32_t> cnt(1025, 0);
        for (uint64_t e = 0; e < m->n_aad; ++e) if (m->aad_aa1[e] < 32 && m->aad_aa2[e] < 32) ++cnt[m->aad_aa1[e] * 32u + m->aad_aa2[e] + 1];
        for (int k = 0; k < 1024; ++k) cnt[k + 1] += cnt[k];
        const size_t base = sd_dist.size();
        sd_dist.resize(base + cnt[1024]); sd_qi.resize(base + cnt[1024]);
        std::vector<uint32_t> cur(cnt.begin(), cnt.end() - 1);
        for (uint64_t e = 0; e < m->n_aad; ++e)
            if (m->aad_aa1[e] < 32 && m->aad_aa2[e] < 32) { const uint32_t k = cur[m->aad_aa1[e] * 32u + m->aad_aa2[e]]++; sd_dist[base + k] = m->aad_dist[e]; sd_qi[base + k] = m->aad_qi[e]; }
        for (int g = 0; g < 1024; ++g) {
            const uint32_t a = cnt[g], b = cnt[g + 1];
            if (b - a < 2) continue;
            grp.clear();
            for (uint32_t k = a; k < b; ++k) grp.emplace_back(sd_dist[base + k], sd_qi[base + k]);
            std::stable_sort(grp.begin(), grp.end(), [](const std::pair<float, uint32_t> &x, const std::pair<float, uint32_t> &y) { return x.first < y.first; });
            for (uint32_t k = a; k < b; ++k) { sd_dist[base + k] = grp[k - a].first; sd_qi[base + k] = grp[k - a].second; }
        }
    }
}

void fd_rh_slot_ranges(const fd_pair_rec *found, uint64_t nf, const fd_cand_rec *cands, const uint32_t *pk_key, uint64_t nc, uint64_t n_cand, size_t *f_lo, size_t *c_lo) {
    size_t fpos = 0, cpos = 0;
    for (uint64_t slot = 0; slot < n_cand; ++slot) {
        f_lo[slot] = fpos; c_lo[slot] = cpos;
        while (fpos < nf && found[fpos].cand == slot) ++fpos;
        if (pk_key) while (cpos < nc && (pk_key[cpos] >> 16) == slot) ++cpos;
        else while (cpos < nc && cands && cands[cpos].cand == slot) ++cpos;
    }
    f_lo[n_cand] = fpos; c_lo[n_cand] = cpos;
}

// ------------------------------------------------------------------------------------------ one slot
namespace {
// the slot's graph with what every component reads of it: the components, the query-map entry of every edge, the edges of every component
struct SlotGraph {
    fd_rh_graph g;
    std::vector<std::vector<uint32_t>> comps, comp_edges;
    std::vector<int32_t> edge_k;      // -1: the hash is not in the map
};
// what a slot allocates once and every component of it reuses (cleared through the touched lists, never refilled)
struct SlotScratch {
    std::vector<uint32_t> votes2, v_touched, q_touched;      // rescue: dense (q, target residue) counters of the component at hand
    std::vector<uint32_t> vote_pos;                          // dense (q, r) -> 1 + vote position of the component at hand
    std::vector<uint32_t> r_mx, r_nmx, r_arg;                // rescue tally per query residue: largest count, its holders, one of them
};
// the slot's candidate pairs bucketed by partner residue j: off[j] .. off[j + 1]) indexes qi / i (records) or, packed, the slot's slice of pk_val
struct CandBuckets { bool have = false, pk = false; std::vector<uint32_t> off, qi, i; };

struct SlotView {      // one slot's share of the call
    const fd_query_map *qm; const std::vector<uint32_t> *e_hash, *e_first; const std::vector<uint64_t> *e_tab; uint32_t e_mask;
    uint32_t q_size, Rt; uint64_t NQ; size_t f0, f1, c0, c1;
};

// graph, components, edge -> map entry, per-component edge lists
void slot_graph(const fd_rh_call &C, const SlotView &V, uint64_t slot, bool big_trace, rh_time s_t0, SlotGraph &G) {
    fd_rh_graph &g = G.g;
    const fd_pair_rec *found = C.found;
    const size_t f0 = V.f0, fpos = V.f1;
    if (fpos - f0 > 256) g.dense.assign((size_t)V.Rt, -1);
    g.es.reserve(fpos - f0); g.et.reserve(fpos - f0); g.eh.reserve(fpos - f0);
    for (size_t e = f0; e < fpos; ++e) {
        uint32_t a = g.node_of(found[e].i), b = g.node_of(found[e].j);
        g.es.push_back(a); g.et.push_back(b); g.eh.push_back(found[e].hash);
    }
    if (big_trace) fprintf(stderr, "[slot %llu] %zu edges: graph at %.3f ms\n", (unsigned long long)slot, fpos - f0, t_ms(s_t0, t_now()));
    G.comps = fd_rh_components(g, C.node_count);
    if (big_trace) fprintf(stderr, "[slot %llu] %zu components at %.3f ms\n", (unsigned long long)slot, G.comps.size(), t_ms(s_t0, t_now()));
    // query-map entry of every found edge, looked up once per candidate (a whole-structure query has ~10^5 entries and
    // thousands of edges per candidate; every component walks the edge list)
    std::vector<int32_t> &edge_k = G.edge_k;
    edge_k.resize(g.es.size());
    if (!V.e_tab->empty()) {
        const std::vector<uint64_t> &T = *V.e_tab;
        const uint32_t msk = V.e_mask;
        for (size_t e = 0; e < g.es.size(); ++e) {
            if (e + 12 < g.es.size()) __builtin_prefetch(&T[(g.eh[e + 12] * 2654435761u) & msk]);      // the table of a whole-structure query is ~2 MB: a miss per probe otherwise
            uint32_t at = (g.eh[e] * 2654435761u) & msk;
            int32_t k = -1;
            while (T[at] != ~0ull) { if ((uint32_t)(T[at] >> 32) == g.eh[e]) { k = (int32_t)(uint32_t)T[at]; break; } at = (at + 1) & msk; }
            edge_k[e] = k;
        }
    } else {
        const std::vector<uint32_t> &e_hash = *V.e_hash, &e_first = *V.e_first;
        for (size_t e = 0; e < g.es.size(); ++e) {
            const auto it = std::lower_bound(e_hash.begin(), e_hash.end(), g.eh[e]);
            edge_k[e] = (it == e_hash.end() || *it != g.eh[e]) ? -1 : (int32_t)e_first[(size_t)(it - e_hash.begin())];
        }
    }
    // the edges of every component, ascending: an edge belongs to a component that holds both its ends (components overlap: a strongly connected set
    // and the weakly connected set around it).  The component loop walked ALL edges per component — 12 components x 12 k edges for a 2,500-residue
    // candidate of a whole-structure query
    const std::vector<std::vector<uint32_t>> &comps = G.comps;
    G.comp_edges.assign(comps.size(), {});
    if (comps.empty()) return;
    const size_t nn = g.w.size();
    std::vector<uint32_t> n_off(nn + 1, 0), n_list;
    for (const auto &cc : comps) for (uint32_t v : cc) ++n_off[v + 1];
    for (size_t v = 0; v < nn; ++v) n_off[v + 1] += n_off[v];
    n_list.resize(n_off[nn]);
    {
        std::vector<uint32_t> cur(n_off.begin(), n_off.end() - 1);
        for (size_t ci = 0; ci < comps.size(); ++ci) for (uint32_t v : comps[ci]) n_list[cur[v]++] = (uint32_t)ci;      // per node: its components, ascending
    }
    for (size_t e = 0; e < g.es.size(); ++e) {
        const uint32_t u = g.es[e], v = g.et[e];
        for (uint32_t x = n_off[u]; x < n_off[u + 1]; ++x)
            for (uint32_t y = n_off[v]; y < n_off[v + 1]; ++y)
                if (n_list[x] == n_list[y]) G.comp_edges[n_list[x]].push_back((uint32_t)e);
    }
}

// one component: votes -> best target per query residue -> greedy assignment; out.q_idx / r_idx / sub_idf (out.rc_ord untouched)
void comp_assign(const SlotView &V, uint32_t htype, const SlotGraph &G, size_t ci, std::vector<uint32_t> &vote_pos, fd_rh_comp_plan &out) {
    const fd_query_map *qm = V.qm;
    const fd_rh_graph &g = G.g;
    const std::vector<int32_t> &edge_k = G.edge_k;
    const std::vector<uint32_t> &cc = G.comps[ci];
    const std::vector<uint32_t> &ce = G.comp_edges[ci];
    const uint32_t q_size = V.q_size;
    std::vector<uint32_t> &q_idx = out.q_idx, &r_idx = out.r_idx;
    q_idx.clear(); r_idx.clear();
    float sub_idf = 0.0f;
    // votes (query residue, target residue) -> saturating u8 count (retrieve.rs:631-666).  Sparse: a component has a
    // handful of edges, the dense q_size x r_size table of the reference is ~1 MB per component for a motif taken
    // from a long chain.  best_c[q] = max count, best_r[q] = smallest target residue holding it (what the
    // reference's running update converges to, counts only grow).
    struct Vote { uint32_t q, r; uint32_t c; };
    std::vector<Vote> votes;
    // (q, r) -> vote: a dense q_size x n_target table when that is small (whole-structure queries against chains of their own
    // size: 10^5 votes per component, a hash map insertion each was most of the component's time), a hash map otherwise (a motif
    // against a long chain: the dense table is ~1 MB per component for a handful of votes)
    const uint32_t n_tr = V.Rt;
    const bool dense_votes = (uint64_t)q_size * n_tr <= (1u << 20) && g.es.size() > 4096;
    if (dense_votes) {
        if (vote_pos.size() < (size_t)q_size * n_tr) vote_pos.assign((size_t)q_size * n_tr, 0u);      // 0 = no vote yet, else 1 + position in votes; cleared below
    }
    std::unordered_map<uint64_t, uint32_t> vote_at;     // (q, r) -> position in votes (first-seen order kept in the vector)
    for (size_t z = 0; z < ce.size(); ++z) {
        const size_t e = ce[z];
        if (z + 16 < ce.size() && edge_k[ce[z + 16]] >= 0) {      // the map's arrays of a whole-structure query are ~1 MB: a miss per edge and array otherwise
            const int32_t k2 = edge_k[ce[z + 16]];
            __builtin_prefetch(&qm->idf[k2]); __builtin_prefetch(&qm->qi[k2]); __builtin_prefetch(&qm->qj[k2]);
        }
        if (edge_k[e] < 0) continue;
        const uint32_t k = (uint32_t)edge_k[e];
        sub_idf += qm->idf[k];                      // calculate_subgraph_idf (retrieve.rs:705-719)
        uint32_t qi = qm->qi[k], qj = qm->qj[k], ri = g.w[g.es[e]], rj = g.w[g.et[e]];
        uint32_t pq[2], pr[2];
        if (fd_hash_is_sym(htype, g.eh[e])) { pq[0] = std::min(qi, qj); pq[1] = std::max(qi, qj); pr[0] = std::min(ri, rj); pr[1] = std::max(ri, rj); }
        else { pq[0] = qi; pr[0] = ri; pq[1] = qj; pr[1] = rj; }
        for (int s = 0; s < 2; ++s) {
            if (dense_votes && pq[s] < q_size && pr[s] < n_tr) {
                uint32_t &slot_v = vote_pos[(size_t)pq[s] * n_tr + pr[s]];
                if (!slot_v) { votes.push_back({pq[s], pr[s], 1u}); slot_v = (uint32_t)votes.size(); }
                else if (votes[slot_v - 1].c < 255) ++votes[slot_v - 1].c;
                continue;
            }
            auto ins = vote_at.emplace(((uint64_t)pq[s] << 32) | pr[s], (uint32_t)votes.size());
            if (ins.second) votes.push_back({pq[s], pr[s], 1u});
            else if (votes[ins.first->second].c < 255) ++votes[ins.first->second].c;
        }
    }
    if (dense_votes) for (const Vote &v : votes) if (v.q < q_size && v.r < n_tr) vote_pos[(size_t)v.q * n_tr + v.r] = 0u;
    struct Best { uint32_t q, c, r; };
    std::vector<Best> best;
    std::unordered_map<uint32_t, uint32_t> best_at;
    for (auto &v : votes) {
        auto ins = best_at.emplace(v.q, (uint32_t)best.size());
        if (ins.second) { best.push_back({v.q, v.c, v.r}); continue; }
        Best *bq = &best[ins.first->second];
        if (v.c > bq->c || (v.c == bq->c && v.r < bq->r)) { bq->c = v.c; bq->r = v.r; }
    }
    // greedy assignment in (count descending, query residue ascending) order (retrieve.rs:668-690)
    std::sort(best.begin(), best.end(), [](const Best &x, const Best &y) { return x.c != y.c ? x.c > y.c : x.q < y.q; });
    for (auto &x : best) {
        if (q_idx.size() == cc.size()) break;
        if (std::find(r_idx.begin(), r_idx.end(), x.r) != r_idx.end()) continue;
        q_idx.push_back(x.q); r_idx.push_back(x.r);
    }
    out.sub_idf = sub_idf;
}

// candidate pairs of this structure bucketed by their partner residue j (counting sort): a component's rescue counts, per
// unmatched query residue, the pairs whose partner the component mapped (retrieve.rs:498-511) — one walk over the
// buckets of its mapped residues instead of one over every pair per query residue (whole-structure queries: millions)
void bucket_cands(const fd_rh_call &C, const SlotView &V, CandBuckets &B) {
    const size_t c0 = V.c0, cpos = V.c1;
    const uint32_t Rt = V.Rt, q_size = V.q_size;
    const fd_cand_rec *cands = C.cands;
    const bool have_c = B.have = cpos > c0, pk = B.pk = C.pk_key != nullptr;
    auto c_ok = [q_size, Rt](const fd_cand_rec &r) { return r.qi < q_size && r.i < Rt && r.j < Rt; };
    B.off.assign(have_c ? Rt + 2 : 2, 0); B.qi.assign(have_c && !pk ? cpos - c0 : 0, 0); B.i.assign(have_c && !pk ? cpos - c0 : 0, 0);
    if (have_c && pk) {   // already sorted by partner residue on the device: the bucket of j is a slice of the packed arrays
        for (size_t e = c0; e < cpos; ++e) { const uint32_t j = C.pk_key[e] & 0xffffu; if (j < Rt) ++B.off[j + 1]; }
        for (uint32_t z = 0; z <= Rt; ++z) B.off[z + 1] += B.off[z];
    } else if (have_c) {
        for (size_t e = c0; e < cpos; ++e) if (c_ok(cands[e])) ++B.off[cands[e].j + 1];
        for (uint32_t z = 0; z <= Rt; ++z) B.off[z + 1] += B.off[z];
        std::vector<uint32_t> cur(B.off.begin(), B.off.end() - 1);
        for (size_t e = c0; e < cpos; ++e) if (c_ok(cands[e])) { uint32_t k = cur[cands[e].j]++; B.qi[k] = cands[e].qi; B.i[k] = cands[e].i; }
    }
}

// rescue votes of one component: (query residue, target residue) -> pairs whose partner is one of its mapped residues, reduced to the tally
void rescue_tally_buckets(const CandBuckets &B, const uint32_t *pk_val_slot, const std::vector<uint32_t> &r_idx, uint32_t q_size, uint32_t Rt, SlotScratch &S) {
    for (uint32_t r : r_idx) {
        if (r >= Rt) continue;
        for (uint32_t z = B.off[r]; z < B.off[r + 1]; ++z) {
            const uint32_t vq = B.pk ? pk_val_slot[z] >> 16 : B.qi[z], vi = B.pk ? pk_val_slot[z] & 0xffffu : B.i[z];
            if (vq >= q_size || vi >= Rt) continue;
            const uint32_t ix2 = vq * Rt + vi;
            if (S.votes2[ix2]++ == 0) S.v_touched.push_back(ix2);
        }
    }
    for (uint32_t ix2 : S.v_touched) {
        const uint32_t vq = ix2 / Rt, vr = ix2 % Rt, vc = S.votes2[ix2];
        if (S.r_mx[vq] == 0) S.q_touched.push_back(vq);
        if (vc > S.r_mx[vq]) { S.r_mx[vq] = vc; S.r_nmx[vq] = 1; S.r_arg[vq] = vr; }
        else if (vc == S.r_mx[vq]) ++S.r_nmx[vq];
        S.votes2[ix2] = 0;
    }
    S.v_touched.clear();
}
// the same three numbers per query residue, counted by the second scan itself
void rescue_tally_rows(const fd_vote_row *vr, uint32_t q_size, SlotScratch &S) {
    for (uint32_t vq = 0; vq < q_size; ++vq)
        if (vr[vq].mx) { S.r_mx[vq] = vr[vq].mx; S.r_nmx[vq] = vr[vq].nmx; S.r_arg[vq] = vr[vq].arg; S.q_touched.push_back(vq); }
}

// residue assignment + rescue (retrieve.rs:430-516): per position of `indices` the from-hash target and the processed one; qs_sc / rs_sc = the
// processed mapping as (query residue, target residue) pairs in the reference's order
void residue_lists(const SlotView &V, const fd_rh_comp_plan &P, const SlotScratch &S, std::vector<int32_t> &from_hash, std::vector<int32_t> &processed,
                   std::vector<uint32_t> &qs_sc, std::vector<uint32_t> &rs_sc) {
    const fd_query_map *qm = V.qm;
    const uint64_t NQ = V.NQ;
    const std::vector<uint32_t> &q_idx = P.q_idx, &r_idx = P.r_idx;
    from_hash.assign(NQ, -1); processed.assign(NQ, -1);
    qs_sc.clear(); rs_sc.clear();
    for (uint64_t pos = 0; pos < NQ; ++pos) {
        uint32_t qi = qm->indices[pos];
        int32_t mapped = -1;
        for (size_t k = 0; k < q_idx.size(); ++k) if (q_idx[k] == qi) { mapped = (int32_t)r_idx[k]; break; }
        if (mapped >= 0) {
            from_hash[pos] = mapped;
            auto itp = std::find(rs_sc.begin(), rs_sc.end(), (uint32_t)mapped);
            if (itp == rs_sc.end()) { processed[pos] = mapped; qs_sc.push_back(qi); rs_sc.push_back((uint32_t)mapped); }
            else {
                size_t pp = (size_t)(itp - rs_sc.begin());
                if (pp < NQ) processed[pp] = -1;   // the reference indexes res_vec with the scanned position
                processed[pos] = mapped;
                qs_sc.erase(qs_sc.begin() + pp); rs_sc.erase(rs_sc.begin() + pp);
                qs_sc.push_back(qi); rs_sc.push_back((uint32_t)mapped);
            }
        } else {
            // the target residue with the unique highest vote (>= 2) joins, unless it is taken (retrieve.rs:498-511)
            if (qi < V.q_size && S.r_nmx[qi] == 1 && S.r_mx[qi] >= 2 && std::find(rs_sc.begin(), rs_sc.end(), S.r_arg[qi]) == rs_sc.end()) {
                processed[pos] = (int32_t)S.r_arg[qi]; qs_sc.push_back(qi); rs_sc.push_back(S.r_arg[qi]);
            }
        }
    }
}

struct SlotCoords { const float *q_ca, *q_cb, *t_ca, *t_cb; };
void add_problem(const SlotCoords &X, const std::vector<uint32_t> &qv, const std::vector<uint32_t> &rv, int which, fd_rh_slot_out &o) {
    for (size_t k = 0; k < qv.size(); ++k) {   // [CA, CB] interleaved (retrieve.rs:761-767)
        for (int z = 0; z < 3; ++z) o.ky.push_back(X.q_ca[3 * qv[k] + z]);
        for (int z = 0; z < 3; ++z) o.ky.push_back(X.q_cb[3 * qv[k] + z]);
        for (int z = 0; z < 3; ++z) o.kx.push_back(X.t_ca[3 * rv[k] + z]);
        for (int z = 0; z < 3; ++z) o.kx.push_back(X.t_cb[3 * rv[k] + z]);
    }
    o.klen.push_back(2 * qv.size());
    o.pend.push_back({o.recs.size() - 1, which});
}
// the component's record, residue lists and Kabsch problems (from-hash mapping; the processed one when it differs)
void emit_record(const SlotCoords &X, uint32_t cand_in_query, const fd_rh_comp_plan &P, const std::vector<int32_t> &from_hash, const std::vector<int32_t> &processed,
                 const std::vector<uint32_t> &qs_sc, const std::vector<uint32_t> &rs_sc, fd_rh_slot_out &o) {
    fd_match_rec rec;
    memset(&rec, 0, sizeof rec);
    rec.cand = cand_in_query; rec.idf = P.sub_idf;
    rec.same = from_hash == processed ? 1 : 0;
    o.recs.push_back(rec);
    o.res.insert(o.res.end(), from_hash.begin(), from_hash.end());
    o.res.insert(o.res.end(), processed.begin(), processed.end());
    add_problem(X, P.q_idx, P.r_idx, 0, o);
    if (!rec.same) add_problem(X, qs_sc, rs_sc, 1, o);
}

// plan pass: a query residue without a target leaves work for the rescue; its votes come from pairs whose partner is mapped.  -> whether the
// component needs the rescue (then its mapped residues are marked under the ordinal n_rc)
bool mark_component(const SlotView &V, const fd_rh_comp_plan &P, uint32_t n_rc, fd_rh_slot_out &o) {
    bool unmatched = false;
    for (uint64_t pos = 0; pos < V.NQ && !unmatched; ++pos) unmatched = std::find(P.q_idx.begin(), P.q_idx.end(), V.qm->indices[pos]) == P.q_idx.end();
    if (!unmatched || P.r_idx.empty()) return false;      // (a component without any mapped residue — a single node under node_count = 1 — has no partner to count votes for and marks nothing)
    for (uint32_t r : P.r_idx) if (r < V.Rt) { o.marks.push_back(r); o.mark_ord.push_back(n_rc); }
    return true;
}
}  // namespace

void fd_rh_slot(const fd_rh_call &C, const uint64_t slot, const bool plan, fd_rh_slot_plan *cache, fd_rh_slot_out &o) {
    const uint64_t tq = C.slot_q[slot];
    SlotView V;
    V.qm = C.qms[tq]; V.e_hash = &C.prep->qhs[tq]; V.e_first = &C.prep->qkf[tq]; V.e_tab = &C.tabs->e_tab[tq]; V.e_mask = C.tabs->e_mask[tq];
    V.q_size = C.prep->q_sizes[tq]; V.NQ = V.qm->n_indices; V.Rt = (uint32_t)(C.g_dst[slot + 1] - C.g_dst[slot]);
    V.f0 = C.f_lo[slot]; V.f1 = C.f_lo[slot + 1]; V.c0 = C.c_lo[slot]; V.c1 = C.c_lo[slot + 1];
    if (V.f1 == V.f0) return;
    const bool cached = !plan && cache && cache->have;
    const bool big_trace = C.trace && V.f1 - V.f0 > 4000;
    const rh_time s_t0 = t_now();
    SlotGraph G;
    if (!cached) slot_graph(C, V, slot, big_trace, s_t0, G);
    const size_t n_comps = cached ? cache->comps.size() : G.comps.size();
    if (big_trace) fprintf(stderr, "[slot %llu] edge entries at %.3f ms (%s)\n", (unsigned long long)slot, t_ms(s_t0, t_now()), plan ? "plan" : "full");
    if (n_comps == 0) return;
    const uint32_t q_size = V.q_size, Rt = V.Rt;
    const SlotCoords X = {C.qb_ca + 3 * C.q_res0[tq], C.qb_cb + 3 * C.q_res0[tq], C.t_all + 3 * C.g_dst[slot], C.t_all + 3 * C.g_total + 3 * C.g_dst[slot]};
    CandBuckets B;
    bucket_cands(C, V, B);
    SlotScratch S;      // allocated once per slot, whatever the number of components
    S.votes2.assign(B.have ? (size_t)q_size * Rt : 0, 0);
    S.r_mx.assign(q_size, 0); S.r_nmx.assign(q_size, 0); S.r_arg.assign(q_size, 0);
    if (plan && cache) { cache->comps.resize(n_comps); cache->have = true; }
    fd_rh_comp_plan own;      // single-scan retrievals keep no plan: one mapping at a time
    std::vector<int32_t> from_hash, processed;
    std::vector<uint32_t> qs_sc, rs_sc;
    uint32_t n_rc = 0;
    for (size_t ci = 0; ci < n_comps; ++ci) {
        fd_rh_comp_plan &P = cache && (plan || cached) ? cache->comps[ci] : own;
        if (!cached) comp_assign(V, C.hash_type, G, ci, S.vote_pos, P);
        if (plan) {
            P.rc_ord = mark_component(V, P, n_rc + 1, o) ? ++n_rc : 0u;
            continue;
        }
        if (B.have) rescue_tally_buckets(B, B.pk ? C.pk_val + V.c0 : nullptr, P.r_idx, q_size, Rt, S);
        if (C.vote_rows && cached && P.rc_ord) rescue_tally_rows(C.vote_rows + C.row_base[slot] + (uint64_t)(P.rc_ord - 1) * q_size, q_size, S);
        residue_lists(V, P, S, from_hash, processed, qs_sc, rs_sc);
        for (uint32_t vq : S.q_touched) { S.r_mx[vq] = 0; S.r_nmx[vq] = 0; }
        S.q_touched.clear();
        emit_record(X, (uint32_t)(slot - C.cand_off[tq]), P, from_hash, processed, qs_sc, rs_sc, o);
    }
    if (big_trace) fprintf(stderr, "[slot %llu] components done at %.3f ms (%s; the slot began %.3f ms into the stage)\n", (unsigned long long)slot, t_ms(s_t0, t_now()), plan ? "plan" : "full", t_ms(C.stage_t0, s_t0));
}

// ------------------------------------------------------------------------------------------ merges, in slot order
void fd_rh_merge_plan(const std::vector<fd_rh_slot_out> &outs, const uint32_t *mask_off, fd_rh_marks &M) {
    for (size_t slot = 0; slot < outs.size(); ++slot) {
        const fd_rh_slot_out &o = outs[slot];
        for (size_t z = 0; z < o.marks.size(); ++z) {
            const uint32_t r = o.marks[z], ord = o.mark_ord[z];
            M.any_rescue = true;
            const uint32_t bit = mask_off[slot] + r;
            M.cj_mask[bit >> 5] |= 1u << (bit & 31u);
            if (ord > 255u || (M.cj_comp[bit] && M.cj_comp[bit] != ord)) M.vote_conflict = true;      // two rescued components share a target residue: host counting
            else M.cj_comp[bit] = (uint8_t)ord;
            M.slot_nrc[slot] = std::max(M.slot_nrc[slot], ord);
        }
    }
}

void fd_rh_merge_full(const std::vector<fd_rh_slot_out> &outs, uint64_t n_queries, const uint64_t *cand_off, fd_rh_merged &R) {
    R.m_off.assign(n_queries + 1, 0); R.r_off.assign(n_queries + 1, 0);
    uint64_t tq = 0;
    for (size_t slot = 0; slot < outs.size(); ++slot) {
        while (slot >= cand_off[tq + 1]) { ++tq; R.m_off[tq] = R.recs.size(); R.r_off[tq] = R.res.size(); }
        const fd_rh_slot_out &o = outs[slot];
        const size_t rec0 = R.recs.size();
        R.recs.insert(R.recs.end(), o.recs.begin(), o.recs.end());
        R.res.insert(R.res.end(), o.res.begin(), o.res.end());
        R.kx.insert(R.kx.end(), o.kx.begin(), o.kx.end());
        R.ky.insert(R.ky.end(), o.ky.begin(), o.ky.end());
        for (uint64_t l : o.klen) R.koff.push_back(R.koff.back() + l);
        for (const fd_rh_pend &pe : o.pend) R.pend.push_back({rec0 + pe.rec, pe.which});
    }
    while (tq < n_queries) { ++tq; R.m_off[tq] = R.recs.size(); R.r_off[tq] = R.res.size(); }
}

// ------------------------------------------------------------------------------------------ test-only entry points (include/fdgpu_debug.h)
// the host glue's graph of found (i, j) residue pairs — nodes in first-appearance order — and its components of at least node_count nodes, as the
// retrieval of > 64-node graphs computes them; and the symmetry flag of hashes.  Pure host code: CPU tests call them without a GPU.
extern "C" int fdgpu_debug_host_components(const uint32_t *edge_i, const uint32_t *edge_j, uint64_t n_edges, uint32_t node_count, uint32_t **residues,
                                           uint64_t **comp_off, uint64_t *n_comps) {
    if ((n_edges && (!edge_i || !edge_j)) || !residues || !comp_off || !n_comps) return FDGPU_EINVAL;
    fd_rh_graph g;
    for (uint64_t e = 0; e < n_edges; ++e) {
        const uint32_t a = g.node_of(edge_i[e]), b = g.node_of(edge_j[e]);
        g.es.push_back(a); g.et.push_back(b); g.eh.push_back(0u);
    }
    const std::vector<std::vector<uint32_t>> comps = fd_rh_components(g, node_count);
    uint64_t tot = 0;
    for (const auto &cc : comps) tot += cc.size();
    uint32_t *r = (uint32_t *)malloc(std::max<uint64_t>(tot, 1) * 4);
    uint64_t *o = (uint64_t *)malloc((comps.size() + 1) * 8);
    if (!r || !o) { free(r); free(o); return FDGPU_ENOMEM; }
    uint64_t w = 0;
    o[0] = 0;
    for (size_t k = 0; k < comps.size(); ++k) { for (uint32_t v : comps[k]) r[w++] = g.w[v]; o[k + 1] = w; }      // a component's nodes ascending, as residues
    *residues = r; *comp_off = o; *n_comps = comps.size();
    return FDGPU_OK;
}
extern "C" int fdgpu_debug_hash_is_symmetric(uint32_t hash_type, const uint32_t *hashes, uint64_t n, uint8_t *out) {
    if (n && (!hashes || !out)) return FDGPU_EINVAL;
    for (uint64_t k = 0; k < n; ++k) out[k] = fd_hash_is_sym(hash_type, hashes[k]) ? 1 : 0;
    return FDGPU_OK;
}

// One candidate slot through fd_rh_slot as the host path of fdgpu_retrieve_batch runs it, from a scan's output given as arrays.  two_pass: the plan
// pass (found triples only), then the candidate pairs the second scan returns — those whose partner residue j the plan pass marked (the scan's
// cj_mask filter, k_match.hip; none at all when nothing was marked: the scan is not run) — then the full pass on the cached plans.
extern "C" int fdgpu_debug_host_retrieve_slot(const uint32_t *found_i, const uint32_t *found_j, const uint32_t *found_hash, uint64_t n_found, const uint32_t *cand_qi,
                                              const uint32_t *cand_i, const uint32_t *cand_j, uint64_t n_pairs, uint32_t n_target, const fd_query_map *qm,
                                              uint32_t hash_type, uint32_t node_count, uint32_t two_pass, uint32_t packed, uint64_t *n_recs, float **idf,
                                              uint32_t **same, int32_t **residues) {
    if ((n_found && (!found_i || !found_j || !found_hash)) || (n_pairs && (!cand_qi || !cand_i || !cand_j)) || !qm || !n_recs || !idf || !same || !residues) return FDGPU_EINVAL;
    for (uint64_t e = 0; e < n_found; ++e) if (found_i[e] >= n_target || found_j[e] >= n_target) return FDGPU_EINVAL;      // a scan emits residues of the candidate only
    if (packed) for (uint64_t e = 0; e < n_pairs; ++e) if ((cand_qi[e] | cand_i[e] | cand_j[e]) >> 16) return FDGPU_EINVAL;   // 16 bits a field
    *n_recs = 0; *idf = nullptr; *same = nullptr; *residues = nullptr;
    fd_rb_prep P;
    fd_rb_prepare(1, &qm, 1.0f, P);
    fd_rh_entry_tabs tabs(1);
    fd_rh_build_e_tab(P, tabs);
    std::vector<fd_pair_rec> found(n_found);
    for (uint64_t e = 0; e < n_found; ++e) found[e] = fd_pair_rec{0u, found_i[e], found_j[e], found_hash[e]};
    const uint64_t cand_off[2] = {0, 1}, g_dst[2] = {0, n_target}, q_res0 = 0;
    const uint32_t slot_q = 0;
    const std::vector<float> t_xyz(std::max<size_t>(6 * (size_t)n_target, 1), 0.0f), q_xyz(3 * (size_t)P.q_sizes[0], 0.0f);      // no superposition here: every point at the origin
    size_t f_lo[2] = {0, (size_t)n_found}, c_lo[2] = {0, 0};
    fd_rh_call C;
    C.qms = &qm; C.prep = &P; C.tabs = &tabs; C.cand_off = cand_off; C.slot_q = &slot_q; C.hash_type = hash_type; C.node_count = node_count;
    C.stage_t0 = std::chrono::steady_clock::now();
    C.found = found.data(); C.f_lo = f_lo; C.c_lo = c_lo;
    C.t_all = t_xyz.data(); C.g_dst = g_dst; C.g_total = n_target; C.qb_ca = q_xyz.data(); C.qb_cb = q_xyz.data(); C.q_res0 = &q_res0;
    fd_rh_slot_plan cache;
    std::vector<char> keep(n_pairs, 1);
    if (two_pass) {
        fd_rh_slot_out po;
        fd_rh_slot(C, 0, true, &cache, po);
        std::vector<char> marked((size_t)n_target + 1, 0);
        for (uint32_t r : po.marks) marked[r] = 1;
        for (uint64_t e = 0; e < n_pairs; ++e) keep[e] = cand_j[e] < n_target && marked[cand_j[e]];
    }
    std::vector<fd_cand_rec> cands;
    std::vector<uint32_t> pk_key, pk_val;
    for (uint64_t e = 0; e < n_pairs; ++e) if (keep[e]) cands.push_back(fd_cand_rec{0u, cand_qi[e], cand_i[e], cand_j[e]});
    if (packed && !cands.empty()) {      // as the scan packs and sorts them: by (slot, partner residue), stable
        std::stable_sort(cands.begin(), cands.end(), [](const fd_cand_rec &a, const fd_cand_rec &b) { return a.j < b.j; });
        for (const fd_cand_rec &r : cands) { pk_key.push_back((r.cand << 16) | (r.j & 0xffffu)); pk_val.push_back((r.qi << 16) | (r.i & 0xffffu)); }
        C.pk_key = pk_key.data(); C.pk_val = pk_val.data();
    } else C.cands = cands.data();
    fd_rh_slot_ranges(found.data(), n_found, C.cands, C.pk_key, cands.size(), 1, f_lo, c_lo);
    std::vector<fd_rh_slot_out> outs(1);
    fd_rh_slot(C, 0, false, two_pass ? &cache : nullptr, outs[0]);
    fd_rh_merged R;
    fd_rh_merge_full(outs, 1, cand_off, R);
    const size_t n = R.recs.size();
    float *o_idf = (float *)malloc(std::max<size_t>(n, 1) * 4);
    uint32_t *o_same = (uint32_t *)malloc(std::max<size_t>(n, 1) * 4);
    int32_t *o_res = (int32_t *)malloc(std::max<size_t>(R.res.size(), 1) * 4);
    if (!o_idf || !o_same || !o_res) { free(o_idf); free(o_same); free(o_res); return FDGPU_ENOMEM; }
    for (size_t k = 0; k < n; ++k) { o_idf[k] = R.recs[k].idf; o_same[k] = R.recs[k].same; }
    if (!R.res.empty()) memcpy(o_res, R.res.data(), R.res.size() * 4);
    *n_recs = n; *idf = o_idf; *same = o_same; *residues = o_res;
    return FDGPU_OK;
}
