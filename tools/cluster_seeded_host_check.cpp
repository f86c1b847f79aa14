// cluster_seeded_host_check.cpp — a stand-alone run of fdgpu_signature_clusters_seeded_host (folddisco_amd/csrc/fd_signatures_host.cpp) for a
// sanitizer build: host C++ alone, no device, no Python.  Built beside the file it checks:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/cluster_seeded_host_check.cpp folddisco_amd/csrc/fd_signatures_host.cpp -o cluster_seeded_host_check && ./cluster_seeded_host_check
//
// Drops and seed tables cut from one table of related records, with sizes around the blocks of the seed scan (64) and of the walk (1,024), in
// several orders and with 1, 3 and 8 threads: every result is checked against a plain sequential walk over combined ids written here.  Without
// seeds the result must be that of fdgpu_signature_clusters_host.  Then every refusal.  Exit status 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>
#include "../include/fdgpu.h"

static const uint32_t EMPTY = 0xffffffffu;

static std::vector<fd_signature> make_table(size_t n, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<fd_signature> t(n);
    for (size_t k = 0; k < n; ++k) {
        fd_signature &g = t[k];
        memset(&g, 0, sizeof g);
        if (k >= 4 && rng() % 3) {                      // most records derive from an earlier one: real groups
            g = t[rng() % k];
            for (unsigned c = rng() % 24; c > 0; --c) g.sk[rng() % 64] = rng() % 5 ? (uint32_t)(rng() % EMPTY) : EMPTY;
            if (rng() % 4) { g.d0 = rng(); g.d1 = rng(); }
        } else {
            for (unsigned b = 0; b < 64; ++b) g.sk[b] = (uint32_t)(rng() % EMPTY);
            g.d0 = rng(); g.d1 = rng();
        }
        g.n = rng() % 11 ? 1 + (uint32_t)(rng() % 5000) : 0;      // empty rows among them, some with a sketch
    }
    return t;
}

static bool nearer(uint32_t mx, uint32_t fx, uint32_t ix, uint32_t my, uint32_t fy, uint32_t iy) {
    const uint32_t l = mx * fy, r = my * fx;
    return l != r ? l > r : fx != fy ? fx > fy : ix < iy;
}

// the definition: the candidates of p are the seeds with n > 0 and the representatives chosen so far, over combined ids
static std::vector<fd_sig_neighbor> walk(const std::vector<fd_signature> &S, const std::vector<uint32_t> &order, const std::vector<fd_signature> &T, uint32_t thr) {
    const uint32_t nT = (uint32_t)T.size();
    std::vector<fd_sig_neighbor> out(S.size(), fd_sig_neighbor{EMPTY, 0, 0, 0});
    std::vector<uint32_t> cand;                         // combined ids
    for (uint32_t j = 0; j < nT; ++j) if (T[j].n) cand.push_back(j);
    for (uint32_t p : order) {
        if (!S[p].n) continue;
        fd_sig_neighbor best{EMPTY, 0, 0, 0};
        for (uint32_t x : cand) {
            const fd_signature &r = x < nT ? T[x] : S[x - nT];
            uint32_t eq = 0, E = 0;
            for (unsigned b = 0; b < 64; ++b) { eq += S[p].sk[b] == r.sk[b]; E += S[p].sk[b] == EMPTY && r.sk[b] == EMPTY; }
            const uint32_t m = eq - E, f = 64 - E;
            if (!f || m * 64 < thr * f || !nearer(m, f, x, best.match, best.filled, best.id)) continue;
            best = fd_sig_neighbor{x, (uint8_t)m, (uint8_t)f, (uint16_t)(S[p].n == r.n && S[p].d0 == r.d0 && S[p].d1 == r.d1)};
        }
        if (best.id == EMPTY) {
            uint32_t filled = 0;
            for (unsigned b = 0; b < 64; ++b) filled += S[p].sk[b] != EMPTY;
            out[p] = fd_sig_neighbor{p, (uint8_t)filled, (uint8_t)filled, FD_SIG_IDENTICAL};
            cand.push_back(nT + p);
            continue;
        }
        if (best.id < nT) best.flags |= FD_SIG_SEED; else best.id -= nT;
        out[p] = best;
    }
    return out;
}

int main() {
    int bad = 0;
    const size_t cells[][2] = {{0, 5}, {1, 0}, {1, 1}, {63, 65}, {64, 64}, {65, 700}, {1023, 64}, {1025, 129}, {2100, 1500}};      // n, nT
    for (const auto &cell : cells) {
        const size_t n = cell[0], nT = cell[1];
        const std::vector<fd_signature> X = make_table(n + nT, 77 + n + 3 * nT);
        std::vector<fd_signature> S, T;                 // alternate records, so groups reach across the two
        for (size_t k = 0; k < n + nT; ++k) (S.size() < n && (k % 2 == 0 || T.size() == nT) ? S : T).push_back(X[k]);
        std::vector<uint32_t> ident(n), rev(n), rnd(n);
        std::iota(ident.begin(), ident.end(), 0u);
        for (size_t k = 0; k < n; ++k) rev[k] = (uint32_t)(n - 1 - k);
        rnd = ident;
        std::mt19937_64 rng(n);
        for (size_t k = n; k > 1; --k) std::swap(rnd[k - 1], rnd[rng() % k]);
        const std::vector<uint32_t> *orders[] = {nullptr, &rev, &rnd};
        size_t of_seeds = 0, of_new = 0;
        for (uint32_t thr : {1u, 32u, 48u, 64u})
            for (const std::vector<uint32_t> *o : orders) {
                const std::vector<fd_sig_neighbor> want = walk(S, o ? *o : ident, T, thr);
                for (size_t p = 0; p < n; ++p) {
                    if (want[p].flags & FD_SIG_SEED) ++of_seeds;
                    else if (want[p].id != EMPTY && want[p].id != p) ++of_new;
                }
                for (uint32_t threads : {1u, 3u, 8u}) {
                    fd_sig_neighbor *got = nullptr;
                    const int rc = fdgpu_signature_clusters_seeded_host(S.data(), n, o ? o->data() : nullptr, T.data(), nT, thr, threads, &got);
                    if (rc != FDGPU_OK || !got || (n && memcmp(got, want.data(), n * sizeof(fd_sig_neighbor)))) {
                        fprintf(stderr, "mismatch: n = %zu, nT = %zu, thr64 = %u, threads = %u, rc = %d\n", n, nT, thr, threads, rc);
                        ++bad;
                    }
                    free(got);
                }
                // without seeds: the unseeded form, byte for byte
                fd_sig_neighbor *plain = nullptr, *none = nullptr;
                const int rc0 = fdgpu_signature_clusters_host(S.data(), n, o ? o->data() : nullptr, thr, 3, &plain);
                const int rc1 = fdgpu_signature_clusters_seeded_host(S.data(), n, o ? o->data() : nullptr, nullptr, 0, thr, 3, &none);
                if (rc0 != FDGPU_OK || rc1 != FDGPU_OK || (n && memcmp(plain, none, n * sizeof(fd_sig_neighbor)))) {
                    fprintf(stderr, "seedless call differs: n = %zu, thr64 = %u\n", n, thr);
                    ++bad;
                }
                free(plain); free(none);
            }
        if (n >= 63 && nT >= 64 && (!of_seeds || !of_new)) { fprintf(stderr, "n = %zu, nT = %zu: a kind of member is missing\n", n, nT); ++bad; }
    }
    const std::vector<fd_signature> S = make_table(65, 5), T = make_table(64, 6);
    std::vector<uint32_t> twice(65), beyond(65);
    std::iota(twice.begin(), twice.end(), 0u);
    beyond = twice;
    twice[7] = 8; beyond[64] = 65;
    fd_sig_neighbor *got = (fd_sig_neighbor *)1;
    const int refused[] = {fdgpu_signature_clusters_seeded_host(S.data(), 65, nullptr, T.data(), 64, 0, 1, &got),
                           fdgpu_signature_clusters_seeded_host(S.data(), 65, nullptr, T.data(), 64, 65, 1, &got),
                           fdgpu_signature_clusters_seeded_host(S.data(), 1ull << 32, nullptr, T.data(), 64, 32, 1, &got),
                           fdgpu_signature_clusters_seeded_host(nullptr, 3, nullptr, T.data(), 64, 32, 1, &got),
                           fdgpu_signature_clusters_seeded_host(S.data(), 65, nullptr, nullptr, 64, 32, 1, &got),
                           fdgpu_signature_clusters_seeded_host(S.data(), 65, nullptr, T.data(), 0xffffffffull - 64, 32, 1, &got),
                           fdgpu_signature_clusters_seeded_host(S.data(), 65, nullptr, T.data(), 1ull << 32, 32, 1, &got),
                           fdgpu_signature_clusters_seeded_host(S.data(), 65, twice.data(), T.data(), 64, 32, 1, &got),
                           fdgpu_signature_clusters_seeded_host(S.data(), 65, beyond.data(), T.data(), 64, 32, 1, &got)};
    for (int rc : refused) bad += rc != FDGPU_EINVAL;
    bad += got != nullptr;
    bad += fdgpu_signature_clusters_seeded_host(S.data(), 65, nullptr, T.data(), 64, 32, 1, nullptr) != FDGPU_EINVAL;
    puts(bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
