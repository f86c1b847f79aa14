// overlap_host_check.cpp — a stand-alone run of fdgpu_rows_intersect_host (folddisco_amd/csrc/fd_overlap_host.cpp) for a sanitizer build:
// host C++ alone, no device, no Python.  Built beside the file it checks:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/overlap_host_check.cpp folddisco_amd/csrc/fd_overlap_host.cpp -o overlap_host_check && ./overlap_host_check
//
// It makes CSR rows of the edge lengths (0, 1, 2, 63 .. 65, 127 .. 129, 192, 1000, 4200; values that reach 0 and 0xFFFFFFFF), intersects
// every pair of them with 1, 3 and 8 threads, inside one set and between two, compares with a std::set_intersection count, and makes every
// refusal.  Exit status 0 and "ok" when all agree.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <random>
#include <vector>
#include "../include/fdgpu.h"

struct csr { std::vector<uint32_t> h; std::vector<uint64_t> off{0}; };

static csr make_rows(uint64_t seed) {
    static const size_t lengths[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 1000, 4200};
    std::mt19937_64 rng(seed);
    std::vector<uint32_t> universe = {0u, 1u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    while (universe.size() < 9000) universe.push_back((uint32_t)rng());
    std::sort(universe.begin(), universe.end());
    universe.erase(std::unique(universe.begin(), universe.end()), universe.end());
    csr r;
    for (int rep = 0; rep < 3; ++rep)
        for (size_t n : lengths) {
            std::vector<uint32_t> row;
            if (rep == 0) row.assign(universe.begin(), universe.begin() + n);                    // a prefix: holds 0
            else if (rep == 1) row.assign(universe.end() - n, universe.end());                   // a suffix: holds 0xFFFFFFFF
            else { row = universe; std::shuffle(row.begin(), row.end(), rng); row.resize(n); std::sort(row.begin(), row.end()); }
            r.h.insert(r.h.end(), row.begin(), row.end());
            r.off.push_back(r.h.size());
        }
    return r;
}

static uint32_t want(const csr &a, uint32_t ka, const csr &b, uint32_t kb) {
    std::vector<uint32_t> out;
    std::set_intersection(a.h.begin() + a.off[ka], a.h.begin() + a.off[ka + 1], b.h.begin() + b.off[kb], b.h.begin() + b.off[kb + 1], std::back_inserter(out));
    return (uint32_t)out.size();
}

int main() {
    int bad = 0;
    const csr A = make_rows(1), B = make_rows(2);
    const uint64_t nA = A.off.size() - 1, nB = B.off.size() - 1;
    for (int two = 0; two < 2; ++two) {
        const csr &S = two ? B : A;
        std::vector<uint32_t> ka, kb, expect;
        for (uint32_t x = 0; x < nA; ++x)
            for (uint32_t y = 0; y < (two ? nB : nA); ++y) { ka.push_back(x); kb.push_back(y); expect.push_back(want(A, x, S, y)); }
        for (uint32_t threads : {0u, 1u, 3u, 8u}) {
            uint32_t *got = nullptr;
            const int rc = fdgpu_rows_intersect_host(A.h.data(), A.off.data(), nA, two ? B.h.data() : nullptr, two ? B.off.data() : nullptr, two ? nB : 0,
                                                     ka.data(), kb.data(), ka.size(), threads, &got);
            if (rc != FDGPU_OK || !got || !std::equal(expect.begin(), expect.end(), got)) {
                fprintf(stderr, "mismatch: two = %d, threads = %u, rc = %d\n", two, threads, rc);
                ++bad;
            }
            free(got);
        }
    }
    uint32_t *got = nullptr;
    bad += fdgpu_rows_intersect_host(nullptr, A.off.data(), 0, nullptr, nullptr, 0, nullptr, nullptr, 0, 1, &got) != FDGPU_OK || !got;      // no row, no pair
    free(got);
    got = (uint32_t *)1;
    const uint32_t k0[] = {0, 5}, k_far[] = {0, (uint32_t)nA};
    std::vector<uint64_t> down(A.off.rbegin(), A.off.rend());
    const int refused[] = {
        fdgpu_rows_intersect_host(A.h.data(), A.off.data(), nA, nullptr, nullptr, 0, k_far, k0, 2, 1, &got),          // a slot at the row count
        fdgpu_rows_intersect_host(A.h.data(), A.off.data(), nA, nullptr, nullptr, 0, k0, k_far, 2, 1, &got),
        fdgpu_rows_intersect_host(A.h.data(), A.off.data(), nA, B.h.data(), B.off.data(), 3, k0, k0, 2, 1, &got),    // 5 is no row of a set of 3
        fdgpu_rows_intersect_host(A.h.data(), A.off.data(), nA, nullptr, nullptr, 0, nullptr, k0, 2, 1, &got),       // a NULL array with a count
        fdgpu_rows_intersect_host(A.h.data(), A.off.data(), nA, nullptr, nullptr, 0, k0, nullptr, 2, 1, &got),
        fdgpu_rows_intersect_host(A.h.data(), nullptr, nA, nullptr, nullptr, 0, k0, k0, 2, 1, &got),
        fdgpu_rows_intersect_host(A.h.data(), A.off.data(), nA, nullptr, nullptr, 0, k0, k0, 1ull << 32, 1, &got),   // refused before anything is read
        fdgpu_rows_intersect_host(A.h.data(), down.data(), nA, nullptr, nullptr, 0, k0, k0, 2, 1, &got)};           // offsets that descend
    for (int rc : refused) bad += rc != FDGPU_EINVAL;
    bad += got != nullptr;
    bad += fdgpu_rows_intersect_host(A.h.data(), A.off.data(), nA, nullptr, nullptr, 0, k0, k0, 2, 1, nullptr) != FDGPU_EINVAL;
    puts(bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
