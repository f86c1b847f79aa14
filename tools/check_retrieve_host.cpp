// The retrieval's host glue (folddisco_amd/csrc/fd_retrieve_host.cpp) on seeded random slots from four threads, for the sanitizers: linked with that
// file alone, CPU only, its own main.  Two queries, four candidate slots each, every slot a different seed:
//   query 0  a few dozen found triples per slot over 80 residues, a map of 60 hashes: sparse votes, bisection, the node map
//   query 1  5,000 found triples per slot over 300 residues, a map of 5,200 hashes: dense graph, dense votes, the hash -> entry table
// Both with symmetric and asymmetric hashes, hashes absent from the map, duplicate `indices`, candidate pairs with out-of-range qi / i / j.
// Four runs over the same slots — single pass and plan-then-full (with the second scan's filter on the candidate pairs in between), each with the
// candidate pairs as records and packed — must give the same records and residue lists: the rescue reads only pairs whose partner is mapped.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tools/check_retrieve_host.cpp folddisco_amd/csrc/fd_retrieve_host.cpp -o check_retrieve_host_asan
//   g++ -O1 -g -std=c++17 -fsanitize=thread -pthread tools/check_retrieve_host.cpp folddisco_amd/csrc/fd_retrieve_host.cpp -o check_retrieve_host_tsan
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <thread>
#include "../folddisco_amd/csrc/fd_retrieve_host.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {      // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 33) % n;
}
// default encoding: residue types at bits 25 and 20, the two torsion (sin, cos) bin pairs in the low byte; symmetric = both pairs of fields equal
static uint32_t make_hash(uint32_t serial, bool sym) {
    const uint32_t a = serial % 20, b = sym ? a : (a + 1 + serial % 7) % 20, t1 = serial % 16, t2 = sym ? t1 : (t1 + 1 + (serial >> 4) % 15) % 16;
    return (a << 25) | (b << 20) | ((serial & 0xfffu) << 8) | (t1 << 4) | t2;
}

struct Query {
    std::vector<uint32_t> hash, qi, qj, indices, aad_qi; std::vector<float> idf, aad_dist; std::vector<uint8_t> prim, aa1, aa2;
    fd_query_map m;
    uint32_t q_size, n_target, n_edges;
};
static void make_query(Query &Q, uint32_t n_hashes, uint32_t q_size, uint32_t n_target, uint32_t n_edges, uint32_t n_indices) {
    Q.q_size = q_size; Q.n_target = n_target; Q.n_edges = n_edges;
    for (uint32_t k = 0; k < n_hashes; ++k) {
        const uint32_t serial = k % (n_hashes - n_hashes / 16);      // the last sixteenth repeats earlier hashes: the first entry wins
        Q.hash.push_back(make_hash(serial, serial % 5 == 0));
        Q.qi.push_back(rnd(q_size)); Q.qj.push_back(rnd(q_size)); Q.idf.push_back((float)(1 + rnd(60)) / 256.0f); Q.prim.push_back(1);
    }
    for (uint32_t k = 0; k < n_indices; ++k) Q.indices.push_back(k % 4 == 3 ? Q.indices[rnd(k)] : rnd(q_size));      // duplicates
    for (uint32_t k = 0; k < 50; ++k) { Q.aa1.push_back((uint8_t)rnd(40)); Q.aa2.push_back((uint8_t)rnd(40)); Q.aad_dist.push_back(4.0f + 0.1f * (float)rnd(100)); Q.aad_qi.push_back(rnd(q_size)); }
    memset(&Q.m, 0, sizeof Q.m);
    Q.m.n = n_hashes; Q.m.hash = Q.hash.data(); Q.m.qi = Q.qi.data(); Q.m.qj = Q.qj.data(); Q.m.is_primary = Q.prim.data(); Q.m.idf = Q.idf.data();
    Q.m.n_indices = n_indices; Q.m.indices = Q.indices.data(); Q.m.primary_hash = Q.hash.data();
    Q.m.n_aad = Q.aad_dist.size(); Q.m.aad_aa1 = Q.aa1.data(); Q.m.aad_aa2 = Q.aa2.data(); Q.m.aad_dist = Q.aad_dist.data(); Q.m.aad_qi = Q.aad_qi.data();
}

struct Run { std::vector<fd_match_rec> recs; std::vector<int32_t> res; std::vector<float> kx, ky; };

int main() {
    const uint64_t n_queries = 2, per = 4, n_cand = n_queries * per;
    Query Q[2];
    make_query(Q[0], 60, 30, 80, 40, 10);
    make_query(Q[1], 5200, 300, 300, 5000, 24);
    const fd_query_map *qms[2] = {&Q[0].m, &Q[1].m};
    fd_rb_prep P;
    fd_rb_prepare(n_queries, qms, 1.0f, P);
    fd_rh_entry_tabs tabs(n_queries);
    fd_rh_build_e_tab(P, tabs);
    std::vector<float> sd_dist; std::vector<uint32_t> sd_qi;
    fd_rh_build_sorted_lists(n_queries, qms, sd_dist, sd_qi);
    if (tabs.e_tab[0].size() != 0 || tabs.e_tab[1].empty() || sd_dist.size() > 100) { printf("FAIL: tables\n"); return 1; }
    // the scans' output, grouped by slot
    std::vector<fd_pair_rec> found;
    std::vector<fd_cand_rec> cands;
    std::vector<uint64_t> cand_off = {0, per, 2 * per}, g_dst(n_cand + 1, 0), q_res0 = {0, Q[0].q_size};
    std::vector<uint32_t> slot_q(n_cand);
    for (uint64_t s = 0; s < n_cand; ++s) {
        const Query &q = Q[s / per];
        slot_q[s] = (uint32_t)(s / per); g_dst[s + 1] = g_dst[s] + q.n_target;
        const uint32_t span = s / per ? q.n_target : 24;      // (small slots: few residues, so that components form)
        for (uint32_t e = 0; e < q.n_edges; ++e) {
            const bool absent = e % 9 == 8;
            const uint32_t i = rnd(span), j = (i + 1 + rnd(span - 1)) % span;
            found.push_back(fd_pair_rec{(uint32_t)s, i, j, absent ? 0xfff00000u + e : q.hash[rnd((uint32_t)q.hash.size())]});
        }
        for (uint32_t e = 0; e < 6 * q.n_edges; ++e) {
            const uint32_t bad = e % 11 == 10 ? 1 + rnd(3) : 0;      // one field out of range, below 2^16: the packed form carries it
            cands.push_back(fd_cand_rec{(uint32_t)s, bad == 1 ? q.q_size + rnd(500) : rnd(q.q_size), bad == 2 ? q.n_target + rnd(500) : rnd(span), bad == 3 ? q.n_target + rnd(500) : rnd(span)});
        }
    }
    const uint64_t g_total = g_dst[n_cand];
    std::vector<float> t_all(6 * g_total), q_xyz(3 * (Q[0].q_size + Q[1].q_size));
    for (float &v : t_all) v = (float)rnd(1000) * 0.05f;
    for (float &v : q_xyz) v = (float)rnd(1000) * 0.05f;
    std::vector<uint32_t> mask_off(n_cand + 1, 0);
    for (uint64_t s = 0; s < n_cand; ++s) mask_off[s] = (uint32_t)g_dst[s];

    Run runs[4];
    for (int form = 0; form < 4; ++form) {
        const bool two_pass = form & 1, packed = form & 2;
        std::vector<size_t> f_lo(n_cand + 1), c_lo(n_cand + 1);
        fd_rh_call C;
        C.qms = qms; C.prep = &P; C.tabs = &tabs; C.cand_off = cand_off.data(); C.slot_q = slot_q.data(); C.hash_type = 3; C.node_count = 2;
        C.stage_t0 = std::chrono::steady_clock::now();
        C.found = found.data(); C.f_lo = f_lo.data(); C.c_lo = c_lo.data();
        C.t_all = t_all.data(); C.g_dst = g_dst.data(); C.g_total = g_total; C.qb_ca = q_xyz.data(); C.qb_cb = q_xyz.data(); C.q_res0 = q_res0.data();
        std::vector<fd_rh_slot_plan> plans(two_pass ? n_cand : 0);
        auto pass = [&](bool plan, std::vector<fd_rh_slot_out> &outs) {
            std::atomic<uint64_t> next(0);
            auto worker = [&]() { for (uint64_t s; (s = next.fetch_add(1)) < n_cand;) fd_rh_slot(C, s, plan, two_pass ? &plans[s] : nullptr, outs[s]); };
            std::vector<std::thread> th;
            for (int t = 0; t < 4; ++t) th.emplace_back(worker);
            for (std::thread &t : th) t.join();
        };
        std::vector<fd_cand_rec> cs = cands;
        if (two_pass) {      // found triples only, then the pairs whose partner residue a component that needs the rescue mapped
            fd_rh_slot_ranges(found.data(), found.size(), nullptr, nullptr, 0, n_cand, f_lo.data(), c_lo.data());
            std::vector<fd_rh_slot_out> pouts(n_cand);
            pass(true, pouts);
            fd_rh_marks M;
            M.cj_mask.assign((g_total + 31) / 32 + 1, 0); M.cj_comp.assign(g_total + 1, 0); M.slot_nrc.assign(n_cand + 1, 0);
            fd_rh_merge_plan(pouts, mask_off.data(), M);
            if (!M.any_rescue) { printf("FAIL: no component needs the rescue\n"); return 1; }
            cs.clear();
            for (const fd_cand_rec &r : cands) {
                const uint32_t nt = (uint32_t)(g_dst[r.cand + 1] - g_dst[r.cand]), bit = mask_off[r.cand] + r.j;
                if (r.j < nt && (M.cj_mask[bit >> 5] >> (bit & 31u)) & 1u) cs.push_back(r);
            }
        } else {      // the records also hold what no scan emits: every field far out of range
            for (uint64_t s = 0; s < n_cand; ++s) cs.insert(std::upper_bound(cs.begin(), cs.end(), (uint32_t)s, [](uint32_t a, const fd_cand_rec &r) { return a < r.cand; }),
                                                            fd_cand_rec{(uint32_t)s, packed ? 65535u : 0xffffffffu, packed ? 65535u : 0xffffffffu, packed ? 65535u : 0xffffffffu});
        }
        std::vector<uint32_t> pk_key, pk_val;
        if (packed) {
            std::stable_sort(cs.begin(), cs.end(), [](const fd_cand_rec &a, const fd_cand_rec &b) { return a.cand != b.cand ? a.cand < b.cand : a.j < b.j; });
            for (const fd_cand_rec &r : cs) { pk_key.push_back((r.cand << 16) | (r.j & 0xffffu)); pk_val.push_back((r.qi << 16) | (r.i & 0xffffu)); }
            C.pk_key = pk_key.data(); C.pk_val = pk_val.data();
        } else C.cands = cs.data();
        fd_rh_slot_ranges(found.data(), found.size(), C.cands, C.pk_key, cs.size(), n_cand, f_lo.data(), c_lo.data());
        if (f_lo[n_cand] != found.size() || c_lo[n_cand] != cs.size()) { printf("FAIL: slot ranges\n"); return 1; }
        std::vector<fd_rh_slot_out> outs(n_cand);
        pass(false, outs);
        fd_rh_merged R;
        fd_rh_merge_full(outs, n_queries, cand_off.data(), R);
        if (R.m_off[n_queries] != R.recs.size() || R.koff.size() != R.pend.size() + 1 || R.kx.size() != 3 * R.koff.back()) { printf("FAIL: merge\n"); return 1; }
        runs[form].recs = R.recs; runs[form].res = R.res; runs[form].kx = R.kx; runs[form].ky = R.ky;
        uint64_t rescued = 0;
        for (const fd_match_rec &r : R.recs) rescued += !r.same;
        printf("form %d (%s, %s): %zu records, %llu with a rescue, %zu candidate pairs\n", form, two_pass ? "plan + full" : "single pass", packed ? "packed" : "records", R.recs.size(),
               (unsigned long long)rescued, cs.size());
        if (R.recs.empty() || !rescued) { printf("FAIL: nothing to compare\n"); return 1; }
    }
    for (int form = 1; form < 4; ++form)
        if (runs[form].recs.size() != runs[0].recs.size() || memcmp(runs[form].recs.data(), runs[0].recs.data(), runs[0].recs.size() * sizeof(fd_match_rec)) != 0 ||
            runs[form].res != runs[0].res || runs[form].kx != runs[0].kx || runs[form].ky != runs[0].ky) { printf("FAIL: form %d differs from form 0\n", form); return 1; }
    printf("OK\n");
    return 0;
}
