// The host steps of make_query_map (folddisco_amd/csrc/fd_query_map_host.cpp) from four threads, for the sanitizers: linked with that file alone (and the
// header-only helper pool), CPU only, its own main.  Every thread runs, serially and with the pooled steps on a pool of its own,
//   a motif-sized call      24 queries of 2 - 9 residues with substitutions: pairs, observed lists, host expansion, first insertions (table), stored fill
//   a whole-structure call  one query of 330 residues (108,570 pairs): pairs, observed list in eight parts, first insertions (radix, and the set form
//                           through its threshold), the implied fill in eight parts
// and compares the pooled results with the serial ones byte for byte.
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tools/check_query_map_host.cpp folddisco_amd/csrc/fd_query_map_host.cpp -o check_query_map_host_asan
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=thread -pthread tools/check_query_map_host.cpp folddisco_amd/csrc/fd_query_map_host.cpp -o check_query_map_host_tsan
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <thread>
#include "../folddisco_amd/csrc/fd_query_map_host.h"

struct Rng {      // xorshift64*, one per thread
    uint64_t s;
    uint32_t operator()(uint32_t n) { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545f4914f6cdd1dull) >> 33) % n; }
};
struct Call {      // a batch's queries and the pair features a device would have returned for them
    std::vector<uint64_t> res_off, q_off; std::vector<uint32_t> q_struct, q_index;
    std::vector<std::vector<uint8_t>> sub_store; std::vector<const uint8_t *> subs; std::vector<uint32_t> n_subs;
    qm_pairs P; std::vector<float> feat; std::vector<uint8_t> valid;
};
static void add_query(Call &C, Rng &rnd, uint32_t s, uint32_t n_res, bool whole, bool with_subs) {
    const uint32_t R = (uint32_t)(C.res_off[s + 1] - C.res_off[s]);
    C.q_struct.push_back(s);
    for (uint32_t k = 0; k < n_res; ++k) {
        C.q_index.push_back(whole ? k : k == 1 ? R : rnd(R));      // a motif query: random residues (repeats happen), one index outside the structure
        C.sub_store.emplace_back();
        if (with_subs && rnd(4) == 0) for (uint32_t a = 0; a < 1 + rnd(3); ++a) C.sub_store.back().push_back((uint8_t)rnd(20));
    }
    C.q_off.push_back(C.q_index.size());
}
static void finish(Call &C, Rng &rnd) {
    for (auto &s : C.sub_store) { C.subs.push_back(s.empty() ? nullptr : s.data()); C.n_subs.push_back((uint32_t)s.size()); }
    qm_list_pairs(C.q_struct.size(), C.q_struct.data(), C.q_off.data(), C.q_index.data(), C.res_off.data(), C.P);
    const size_t np = C.P.pi.size();
    C.feat.resize(np * FD_QF); C.valid.resize(np);
    for (size_t k = 0; k < np; ++k) {
        C.valid[k] = rnd(5) != 0;
        float *f = &C.feat[k * FD_QF];
        for (int z = 0; z < FD_QF; ++z) f[z] = 0.001f * (float)rnd(25000) - (z >= 4 && z < 9 ? 3.0f : 0.0f);
        f[0] = f[10] = (float)rnd(20); f[1] = f[11] = (float)rnd(20);
    }
}
#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "check_query_map_host: %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)
static bool same_aad(const qm_aad &a, const qm_aad &b) { return a.a1 == b.a1 && a.a2 == b.a2 && a.aq == b.aq && a.ad.size() == b.ad.size() && !memcmp(a.ad.data(), b.ad.data(), a.ad.size() * 4); }
static bool same_map(const fd_query_map *a, const fd_query_map *b) {      // one block each: the arrays sit at equal offsets, compare them through the struct
    if (a->n != b->n || a->arena_bytes != b->arena_bytes || a->n_aad != b->n_aad || a->n_indices != b->n_indices) return false;
    return !memcmp(a->hash, b->hash, a->n * 4) && !memcmp(a->qi, b->qi, a->n * 4) && !memcmp(a->qj, b->qj, a->n * 4) && !memcmp(a->idf, b->idf, a->n * 4) &&
           !memcmp(a->primary_hash, b->primary_hash, a->n * 4) && !memcmp(a->is_primary, b->is_primary, a->n) && !memcmp(a->aad_dist, b->aad_dist, a->n_aad * 4) &&
           !memcmp(a->indices, b->indices, a->n_indices * 4) && (!a->post_len || !memcmp(a->post_len, b->post_len, a->n * 8));
}

// host form: expansion with substitutions, table dedupe, stored fill — per query; pool: also the observed lists through it
static int motif_call(Rng &rnd, fd_host_pool *pool, std::vector<fd_query_map *> &maps) {
    Call C;
    C.res_off = {0, 40, 100, 130}; C.q_off = {0};
    for (uint32_t t = 0; t < 24; ++t) add_query(C, rnd, t % 3, 2 + rnd(8), false, true);
    finish(C, rnd);
    const qm_feat F = {C.feat.data(), C.valid.data()};
    const float dthr[2] = {0.5f, 0.3f}, athr[1] = {0.0872665f};
    qm_cands cands;
    std::vector<uint64_t> cand_off(1, 0), tab;
    std::vector<qm_aad> aads(24);
    for (uint32_t t = 0; t < 24; ++t) {
        const uint64_t a = C.q_off[t], r0 = C.res_off[C.q_struct[t]];
        qm_observed_list(F, C.P.pi.data(), C.P.off[t], C.P.off[t + 1], r0, pool, 4, aads[t]);
        qm_expand_query(F, C.P.pi.data(), C.P.pj.data(), C.P.off[t], C.P.off[t + 1], r0, C.q_index.data() + a, C.q_off[t + 1] - a, C.subs.data() + a, C.n_subs.data() + a,
                        qm_fields_of(3), qm_thresholds{dthr, 2, athr, 1}, cands);
        cand_off.push_back(cands.c.size());
    }
    std::vector<uint32_t> hashes(cands.c.size() + 1), pair_primary(C.P.pi.size() + 1, 7u);
    std::vector<float> pair_idf(C.P.pi.size() + 1, 1.5f);
    for (size_t z = 0; z < cands.c.size(); ++z) hashes[z] = (uint32_t)(cands.vf[z * FD_QF + 2] * 4.0f) * 2654435761u;      // a few hundred values: repeats
    const uint32_t *planes[1] = {hashes.data()};
    for (uint32_t t = 0; t < 24; ++t) {
        const qm_insertions I = {planes, 1, cand_off[t], cand_off[t + 1] - cand_off[t]};
        std::vector<uint32_t> keep;
        qm_first_wins(I, tab, keep);
        REQUIRE(I.n_ins == 0 || (!keep.empty() && keep[0] == 0));
        const qm_map_src S = {keep.data(), keep.size(), I, cands.c.data(), nullptr, 0, C.P.pi.data(), C.P.pj.data(), C.res_off[C.q_struct[t]], pair_idf.data(), pair_primary.data(),
                              nullptr, nullptr, nullptr, 0, C.q_index.data() + C.q_off[t], (size_t)(C.q_off[t + 1] - C.q_off[t]), &aads[t]};
        maps.push_back(qm_fill_map(S, pool, 4));
        REQUIRE(maps.back());
    }
    return 0;
}
// device forms' host side for one whole-structure query: observed list and implied fill in eight parts, radix and set dedupe
static int whole_call(Rng &rnd, fd_host_pool *pool, std::vector<fd_query_map *> &maps) {
    Call C;
    C.res_off = {0, 25, 355}; C.q_off = {0};
    add_query(C, rnd, 1, 330, true, false);
    finish(C, rnd);
    const size_t np = C.P.pi.size();
    REQUIRE(np == 330u * 329u);
    const qm_feat F = {C.feat.data(), C.valid.data()};
    qm_aad aad;
    qm_observed_list(F, C.P.pi.data(), 0, np, 25, pool, 4, aad);
    qm_aad serial;
    qm_observed_list(F, C.P.pi.data(), 0, np, 25, nullptr, 1, serial);
    REQUIRE(same_aad(aad, serial));
    std::vector<uint32_t> vpairs;
    for (size_t k = 0; k < np; ++k) if (C.valid[k]) vpairs.push_back((uint32_t)k);
    const uint64_t pp = 3, nc = vpairs.size() * pp;
    std::vector<uint32_t> hashes(nc), pair_primary(np, 0u);
    std::vector<float> pair_idf(np, 0.25f);
    for (uint64_t z = 0; z < nc; ++z) hashes[z] = rnd(60000) * 2654435761u;
    const uint32_t *planes[1] = {hashes.data()};
    const qm_insertions I = {planes, 1, 0, nc};
    std::vector<uint64_t> tab;
    std::vector<uint32_t> keep, keep_set;
    qm_first_wins(I, tab, keep);
    qm_first_wins(I, tab, keep_set, 16, 17);
    REQUIRE(keep == keep_set && keep.size() > 16384 && keep.size() <= 60000);
    std::vector<uint64_t> post_len(keep.size(), 3); std::vector<uint32_t> post_seg(keep.size(), 1); std::vector<long long> post_kidx(keep.size(), -1);
    const qm_map_src S = {keep.data(), keep.size(), I, nullptr, vpairs.data(), pp, C.P.pi.data(), C.P.pj.data(), 25, pair_idf.data(), pair_primary.data(),
                          post_len.data(), post_seg.data(), post_kidx.data(), 9, C.q_index.data(), C.q_index.size(), &aad};
    maps.push_back(qm_fill_map(S, pool, 4));
    REQUIRE(maps.back());
    return 0;
}
static int one_thread(uint64_t seed) {
    std::vector<fd_query_map *> serial, pooled;
    {
        fd_host_pool pool;
        Rng a = {seed}, b = {seed};
        if (motif_call(a, nullptr, serial) || motif_call(b, &pool, pooled) || whole_call(a, nullptr, serial) || whole_call(b, &pool, pooled)) return 1;
    }
    REQUIRE(serial.size() == 25 && pooled.size() == 25);
    for (size_t t = 0; t < serial.size(); ++t) { REQUIRE(same_map(serial[t], pooled[t])); free(serial[t]); free(pooled[t]); }
    return 0;
}
int main() {
    std::atomic<int> bad(0);
    std::vector<std::thread> th;
    for (int t = 0; t < 4; ++t) th.emplace_back([&bad, t] { bad += one_thread(0x9e3779b97f4a7c15ull * (uint64_t)(t + 1)); });
    for (auto &x : th) x.join();
    printf("check_query_map_host: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
