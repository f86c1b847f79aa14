// exact_neighbors_host_check.cpp — a stand-alone run of fdgpu_rows_neighbors_host (folddisco_amd/csrc/fd_neighbors_exact_host.cpp) for a
// sanitizer build: host C++ alone, no device, no Python.  Built beside the file it checks:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/exact_neighbors_host_check.cpp folddisco_amd/csrc/fd_neighbors_exact_host.cpp -o exact_neighbors_host_check && ./exact_neighbors_host_check
//
// It makes 300 rows over a universe that reaches 0 and 0xFFFFFFFF (empty rows, twins, rows of the chunk-edge lengths, a hash every row holds),
// transposes them to an index at the first ids 0 and 16200, ranks every query against every row by std::set_intersection and a full sort under
// the order of include/fdgpu.h, compares with the library for 0, 1, 3 and 8 threads, every k of 1, 8 and 32 and the floors 0, 1, 5000 and
// 10000, with and without the exclusion, and makes every refusal.  Exit status 0 and "ok" when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <random>
#include <vector>
#include "../include/fdgpu.h"

typedef std::vector<std::vector<uint32_t>> rows_t;
struct csr { std::vector<uint32_t> h; std::vector<uint64_t> off{0}; };
struct index_t { std::vector<uint32_t> hashes; std::vector<uint64_t> offsets{0}; std::vector<uint8_t> value; };

static rows_t make_rows(uint64_t seed) {
    static const size_t lengths[] = {0, 1, 63, 64, 65, 128, 129, 1000};
    std::mt19937_64 rng(seed);
    std::vector<uint32_t> universe = {0u, 1u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    while (universe.size() < 3000) universe.push_back((uint32_t)rng());
    std::sort(universe.begin(), universe.end());
    universe.erase(std::unique(universe.begin(), universe.end()), universe.end());
    rows_t rows;
    for (int k = 0; k < 300; ++k) {
        std::vector<uint32_t> row;
        if (k % 50 == 49) { rows.push_back(rows[k - 1]); continue; }                            // a twin of the row before
        const size_t n = k < 8 ? lengths[k] : k % 37 == 0 ? 0 : 1 + rng() % 200;
        row = universe;
        std::shuffle(row.begin(), row.end(), rng);
        row.resize(n);
        if (n > 1 && k % 3) { row.push_back(0u); row.push_back(0xFFFFFFFFu); row.push_back(universe[7]); }      // hashes most rows hold: long lists
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end()), row.end());
        rows.push_back(row);
    }
    return rows;
}

static csr to_csr(const rows_t &rows) {
    csr r;
    for (const auto &row : rows) { r.h.insert(r.h.end(), row.begin(), row.end()); r.off.push_back(r.h.size()); }
    return r;
}

static index_t transpose(const rows_t &rows, uint32_t first_id) {
    std::map<uint32_t, std::vector<uint32_t>> lists;
    for (size_t s = 0; s < rows.size(); ++s) for (uint32_t h : rows[s]) lists[h].push_back(first_id + (uint32_t)s);
    index_t ix;
    for (const auto &kv : lists) {
        ix.hashes.push_back(kv.first);
        uint32_t prev = 0;
        for (uint32_t id : kv.second) {
            uint32_t v = id - prev;
            prev = id;
            do { uint8_t b = v & 0x7f; v >>= 7; ix.value.push_back(b | (v ? 0x80 : 0)); } while (v);
        }
        ix.offsets.push_back(ix.value.size());
    }
    return ix;
}

static bool nearer(const fd_row_neighbor &x, const fd_row_neighbor &y) {
    const uint64_t l = (uint64_t)x.inter * y.uni, r = (uint64_t)y.inter * x.uni;
    return l != r ? l > r : x.inter != y.inter ? x.inter > y.inter : x.id < y.id;
}

// |Q[q] ∩ D[s]| for every pair, by std::set_intersection
static std::vector<std::vector<uint32_t>> intersections(const rows_t &Q, const rows_t &D) {
    std::vector<std::vector<uint32_t>> m(Q.size(), std::vector<uint32_t>(D.size(), 0u));
    for (size_t q = 0; q < Q.size(); ++q)
        for (size_t s = 0; s < D.size(); ++s) {
            std::vector<uint32_t> both;
            std::set_intersection(Q[q].begin(), Q[q].end(), D[s].begin(), D[s].end(), std::back_inserter(both));
            m[q][s] = (uint32_t)both.size();
        }
    return m;
}

static std::vector<fd_row_neighbor> brute(const rows_t &Q, const rows_t &D, const std::vector<std::vector<uint32_t>> &m, uint32_t first_id, const uint32_t *exclude,
                                          uint32_t k, uint32_t T) {
    std::vector<fd_row_neighbor> out(Q.size() * k, fd_row_neighbor{0xFFFFFFFFu, 0, 0, 0});
    for (size_t q = 0; q < Q.size(); ++q) {
        std::vector<fd_row_neighbor> c;
        for (size_t s = 0; s < D.size(); ++s) {
            const uint32_t inter = m[q][s], uni = (uint32_t)(Q[q].size() + D[s].size() - inter), id = first_id + (uint32_t)s;
            if (!inter || (exclude && exclude[q] == id) || (uint64_t)inter * 10000 < (uint64_t)T * uni) continue;
            c.push_back(fd_row_neighbor{id, inter, uni, inter == Q[q].size() && inter == D[s].size() ? FD_ROW_EQUAL : 0u});
        }
        std::sort(c.begin(), c.end(), nearer);
        for (size_t r = 0; r < c.size() && r < k; ++r) out[q * k + r] = c[r];
    }
    return out;
}

int main() {
    int bad = 0;
    const rows_t D = make_rows(1), A = make_rows(2);
    std::vector<uint32_t> d_len;
    for (const auto &r : D) d_len.push_back((uint32_t)r.size());
    const std::vector<std::vector<uint32_t>> m_own = intersections(D, D), m_other = intersections(A, D);
    for (uint32_t first_id : {0u, 16200u}) {
        const index_t ix = transpose(D, first_id);
        for (int two = 0; two < 2; ++two) {              // the index's own rows as queries (each one's id excluded), then those of another set
            const rows_t &Q = two ? A : D;
            const csr q = to_csr(Q);
            std::vector<uint32_t> excl;
            for (size_t s = 0; s < Q.size(); ++s) excl.push_back(first_id + (uint32_t)s);
            const uint32_t *ex = two ? nullptr : excl.data();
            for (uint32_t k : {1u, 8u, 32u})
                for (uint32_t T : {0u, 1u, 5000u, 10000u}) {
                    const std::vector<fd_row_neighbor> want = brute(Q, D, two ? m_other : m_own, first_id, ex, k, T);
                    for (uint32_t threads : {0u, 1u, 3u, 8u}) {
                        fd_row_neighbor *got = nullptr;
                        const int rc = fdgpu_rows_neighbors_host(q.h.data(), q.off.data(), Q.size(), ix.hashes.data(), ix.offsets.data(), ix.hashes.size(), ix.value.data(),
                                                                 ix.value.size(), first_id, D.size(), d_len.data(), ex, k, T, threads, &got);
                        if (rc != FDGPU_OK || !got || memcmp(got, want.data(), want.size() * sizeof(fd_row_neighbor))) {
                            fprintf(stderr, "mismatch: first_id = %u, two = %d, k = %u, floor = %u, threads = %u, rc = %d\n", first_id, two, k, T, threads, rc);
                            ++bad;
                        }
                        free(got);
                    }
                }
        }
    }
    const index_t ix = transpose(D, 16200);
    const csr q = to_csr(D);
    const uint64_t nQ = D.size(), S = D.size(), H = ix.hashes.size(), V = ix.value.size();
    fd_row_neighbor *got = nullptr;
    bad += fdgpu_rows_neighbors_host(nullptr, q.off.data(), 0, ix.hashes.data(), ix.offsets.data(), H, ix.value.data(), V, 16200, S, d_len.data(), nullptr, 8, 0, 1, &got) != FDGPU_OK || !got;
    free(got);                                           // no query: an empty result
    got = (fd_row_neighbor *)1;
    std::vector<uint32_t> ex_low(nQ, 0xFFFFFFFFu), ex_high(nQ, 0xFFFFFFFFu), low = d_len;
    ex_low[3] = 16199; ex_high[nQ - 1] = 16200 + (uint32_t)S;
    low[48] -= 1;                                        // row 49 is its twin: it shares more hashes than this length allows
    std::vector<uint64_t> down(q.off.rbegin(), q.off.rend()), swapped = ix.offsets;
    std::swap(swapped[5], swapped[6]);
    std::vector<uint8_t> far = ix.value, cut = ix.value;
    far[ix.offsets[1] - 1] = 0x7f;                       // the last delta of the first list: an id beyond the index
    cut[ix.offsets[1] - 1] |= 0x80;                      // the first list ends inside a varint
#define CALL(qh, qo, dv, doff, dl, ex, k, T, fid, out) fdgpu_rows_neighbors_host(qh, qo, nQ, ix.hashes.data(), doff, H, dv, V, fid, S, dl, ex, k, T, 1, out)
    const int refused[] = {
        CALL(q.h.data(), q.off.data(), ix.value.data(), ix.offsets.data(), d_len.data(), nullptr, 0, 0, 16200, &got),           // k outside 1 .. 32
        CALL(q.h.data(), q.off.data(), ix.value.data(), ix.offsets.data(), d_len.data(), nullptr, 33, 0, 16200, &got),
        CALL(q.h.data(), q.off.data(), ix.value.data(), ix.offsets.data(), d_len.data(), nullptr, 8, 10001, 16200, &got),       // the floor above 10000
        CALL(q.h.data(), q.off.data(), ix.value.data(), ix.offsets.data(), nullptr, nullptr, 8, 0, 16200, &got),                // d_len NULL with S > 0
        CALL(q.h.data(), nullptr, ix.value.data(), ix.offsets.data(), d_len.data(), nullptr, 8, 0, 16200, &got),                // the queries NULL
        CALL(nullptr, q.off.data(), ix.value.data(), ix.offsets.data(), d_len.data(), nullptr, 8, 0, 16200, &got),
        CALL(q.h.data(), q.off.data(), nullptr, ix.offsets.data(), d_len.data(), nullptr, 8, 0, 16200, &got),                   // the index NULL
        CALL(q.h.data(), q.off.data(), ix.value.data(), nullptr, d_len.data(), nullptr, 8, 0, 16200, &got),
        CALL(q.h.data(), q.off.data(), ix.value.data(), ix.offsets.data(), d_len.data(), ex_low.data(), 8, 0, 16200, &got),     // an exclude id outside the index
        CALL(q.h.data(), q.off.data(), ix.value.data(), ix.offsets.data(), d_len.data(), ex_high.data(), 8, 0, 16200, &got),
        CALL(q.h.data(), down.data(), ix.value.data(), ix.offsets.data(), d_len.data(), nullptr, 8, 0, 16200, &got),            // offsets that descend
        CALL(q.h.data(), q.off.data(), ix.value.data(), ix.offsets.data(), d_len.data(), nullptr, 8, 0, 0xFFFFFFFFull, &got),   // ids that leave 32 bits
        CALL(q.h.data(), q.off.data(), ix.value.data(), ix.offsets.data(), low.data(), nullptr, 8, 0, 16200, &got),             // lengths of another index
        CALL(q.h.data(), q.off.data(), ix.value.data(), swapped.data(), d_len.data(), nullptr, 8, 0, 16200, &got),              // a damaged index
        CALL(q.h.data(), q.off.data(), far.data(), ix.offsets.data(), d_len.data(), nullptr, 8, 0, 16200, &got),
        CALL(q.h.data(), q.off.data(), cut.data(), ix.offsets.data(), d_len.data(), nullptr, 8, 0, 16200, &got)};
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; ++i)
        if (refused[i] != FDGPU_EINVAL) { fprintf(stderr, "refusal %zu: rc = %d\n", i, refused[i]); ++bad; }
    bad += got != nullptr;
    bad += CALL(q.h.data(), q.off.data(), ix.value.data(), ix.offsets.data(), d_len.data(), nullptr, 8, 0, 16200, nullptr) != FDGPU_EINVAL;
    puts(bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
