// The pair scan's host tables (folddisco_amd/csrc/fd_match_tables.cpp) from four threads, for the sanitizers: linked with that file alone (and the
// header-only helper pool), CPU only, its own main.  Every thread builds and packs, serial and through a pool of its own,
//   a motif-sized call      64 queries of a dozen observed distances and 40 hashes, 8 candidates each, both item forms
//   a whole-structure call  one query of 30,000 observed distances (interval tables, eight parts on the pool) and 20,000 hashes (a hash set), 20 candidates
// and compares the pooled block with the serial one byte for byte.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tools/check_match_tables.cpp folddisco_amd/csrc/fd_match_tables.cpp -o check_match_tables_asan
//   g++ -O1 -g -std=c++17 -fsanitize=thread -pthread tools/check_match_tables.cpp folddisco_amd/csrc/fd_match_tables.cpp -o check_match_tables_tsan
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <thread>
#include "../folddisco_amd/csrc/fd_match_tables.h"

struct Rng {      // xorshift64*, one per thread
    uint64_t s;
    uint32_t operator()(uint32_t n) { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)((s * 0x2545f4914f6cdd1dull) >> 33) % n; }
};
struct Query {
    std::vector<uint32_t> hashes, qi; std::vector<uint8_t> aa1, aa2; std::vector<float> dist;
    fd_match_query q;
};
static void make_query(Query &Q, Rng &rnd, uint32_t n_hashes, uint32_t n_aad, float window) {
    for (uint32_t k = 0; k < n_hashes; ++k) Q.hashes.push_back((rnd(20) << 25) | (rnd(20) << 20) | k);      // default encoding: residue types at bits 25 and 20
    for (uint32_t k = 0; k < n_aad; ++k) {
        Q.aa1.push_back((uint8_t)(k % 97 == 0 ? 255 : rnd(20))); Q.aa2.push_back((uint8_t)rnd(20));      // a few entries without a residue type
        Q.dist.push_back(3.0f + 0.001f * (float)rnd(17000)); Q.qi.push_back(rnd(300));
    }
    Q.q = fd_match_query{Q.hashes.data(), Q.hashes.size(), Q.aa1.data(), Q.aa2.data(), Q.dist.data(), Q.qi.data(), Q.dist.size(), window, n_hashes <= 200};
}

// one call's tables, packed into a zeroed block; 0 = built
static int build(const std::vector<Query> &qs, uint32_t per_query, const std::vector<uint64_t> &res_off, bool dev_items, fd_host_pool *pool, Rng &rnd,
                 std::vector<uint32_t> &blk) {
    std::vector<fd_match_query> mq;
    std::vector<uint32_t> cand;
    std::vector<uint64_t> cand_off(1, 0);
    for (const Query &Q : qs) {
        mq.push_back(Q.q);
        for (uint32_t k = 0; k < per_query; ++k) cand.push_back(rnd((uint32_t)res_off.size() - 1));
        cand_off.push_back(cand.size());
    }
    const mp_tables_in in = {qs.size(), mq.data(), cand.data(), cand_off.data(), res_off.data(), res_off.size() - 1, 3u, dev_items};
    mp_built B;
    fd_mp_tables TB;
    const char *msg = nullptr;
    if (mp_build_tables(in, pool, B, TB, &msg)) { fprintf(stderr, "refused: %s\n", msg); return 1; }
    blk.assign(TB.L.words, 0);
    mp_pack(in, TB.L, B, blk.data());
    return 0;
}

int main() {
    std::atomic<int> bad(0);
    auto worker = [&](unsigned id) {
        Rng rnd{0x9e3779b97f4a7c15ull + id};
        std::vector<uint64_t> res_off(1, 0);
        for (int s = 0; s < 40; ++s) res_off.push_back(res_off.back() + (s % 7 == 0 ? 0 : 30 + rnd(600)));      // some empty structures
        std::vector<Query> motif(64), whole(1);
        for (Query &Q : motif) make_query(Q, rnd, 40, 12, 1.0f);
        make_query(whole[0], rnd, 20000, 30000, 1.0f);
        fd_host_pool pool;
        for (int form = 0; form < 3; ++form) {      // motif call with device-written items, with host-built items, the whole-structure call
            const std::vector<Query> &qs = form < 2 ? motif : whole;
            std::vector<uint32_t> serial, pooled;
            const Rng at = rnd;
            Rng r1 = at, r2 = at;
            if (build(qs, form < 2 ? 8 : 20, res_off, form == 0, nullptr, r1, serial) || build(qs, form < 2 ? 8 : 20, res_off, form == 0, &pool, r2, pooled)) { ++bad; return; }
            if (serial.size() != pooled.size() || memcmp(serial.data(), pooled.data(), serial.size() * 4)) { fprintf(stderr, "thread %u form %d: pooled block differs\n", id, form); ++bad; }
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 0; t < 4; ++t) th.emplace_back(worker, t);
    for (auto &t : th) t.join();
    printf(bad ? "FAILED\n" : "check_match_tables: ok\n");
    return bad ? 1 : 0;
}
