// cluster_host_check.cpp — a stand-alone run of fdgpu_signature_clusters_host (folddisco_amd/csrc/fd_signatures_host.cpp) for a sanitizer
// build: host C++ alone, no device, no Python.  Built beside the file it checks:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/cluster_host_check.cpp folddisco_amd/csrc/fd_signatures_host.cpp -o cluster_host_check && ./cluster_host_check
//
// It walks tables whose sizes straddle the host form's block of 1,024 positions in several orders, with 1, 3 and 8 threads, checks every result
// against a plain sequential walk written here, and makes every refusal.  Exit status 0 and "ok" when all agree.
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

static std::vector<fd_sig_neighbor> walk(const std::vector<fd_signature> &S, const std::vector<uint32_t> &order, uint32_t thr) {
    std::vector<fd_sig_neighbor> out(S.size(), fd_sig_neighbor{EMPTY, 0, 0, 0});
    std::vector<uint32_t> reps;
    for (uint32_t p : order) {
        if (!S[p].n) continue;
        fd_sig_neighbor best{EMPTY, 0, 0, 0};
        for (uint32_t r : reps) {
            uint32_t eq = 0, E = 0;
            for (unsigned b = 0; b < 64; ++b) { eq += S[p].sk[b] == S[r].sk[b]; E += S[p].sk[b] == EMPTY && S[r].sk[b] == EMPTY; }
            const uint32_t m = eq - E, f = 64 - E;
            if (!f || m * 64 < thr * f || !nearer(m, f, r, best.match, best.filled, best.id)) continue;
            best = fd_sig_neighbor{r, (uint8_t)m, (uint8_t)f, (uint16_t)(S[p].n == S[r].n && S[p].d0 == S[r].d0 && S[p].d1 == S[r].d1)};
        }
        if (best.id == EMPTY) {
            uint32_t filled = 0;
            for (unsigned b = 0; b < 64; ++b) filled += S[p].sk[b] != EMPTY;
            best = fd_sig_neighbor{p, (uint8_t)filled, (uint8_t)filled, FD_SIG_IDENTICAL};
            reps.push_back(p);
        }
        out[p] = best;
    }
    return out;
}

int main() {
    int bad = 0;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)1023, (size_t)1024, (size_t)1025, (size_t)3000}) {
        const std::vector<fd_signature> S = make_table(n, 99 + n);
        std::vector<uint32_t> ident(n), rev(n), rnd(n);
        std::iota(ident.begin(), ident.end(), 0u);
        for (size_t k = 0; k < n; ++k) rev[k] = (uint32_t)(n - 1 - k);
        rnd = ident;
        std::mt19937_64 rng(n);
        for (size_t k = n; k > 1; --k) std::swap(rnd[k - 1], rnd[rng() % k]);
        const std::vector<uint32_t> *orders[] = {nullptr, &ident, &rev, &rnd};
        for (uint32_t thr : {1u, 32u, 48u, 64u})
            for (const std::vector<uint32_t> *o : orders) {
                const std::vector<fd_sig_neighbor> want = walk(S, o ? *o : ident, thr);
                for (uint32_t threads : {1u, 3u, 8u}) {
                    fd_sig_neighbor *got = nullptr;
                    const int rc = fdgpu_signature_clusters_host(S.data(), n, o ? o->data() : nullptr, thr, threads, &got);
                    if (rc != FDGPU_OK || !got || (n && memcmp(got, want.data(), n * sizeof(fd_sig_neighbor)))) {
                        fprintf(stderr, "mismatch: n = %zu, thr64 = %u, threads = %u, rc = %d\n", n, thr, threads, rc);
                        ++bad;
                    }
                    free(got);
                }
            }
    }
    const std::vector<fd_signature> S = make_table(65, 5);
    std::vector<uint32_t> twice(65), beyond(65);
    std::iota(twice.begin(), twice.end(), 0u);
    beyond = twice;
    twice[7] = 8; beyond[64] = 65;
    fd_sig_neighbor *got = (fd_sig_neighbor *)1;
    const int refused[] = {fdgpu_signature_clusters_host(S.data(), 65, nullptr, 0, 1, &got), fdgpu_signature_clusters_host(S.data(), 65, nullptr, 65, 1, &got),
                           fdgpu_signature_clusters_host(S.data(), 1ull << 32, nullptr, 32, 1, &got), fdgpu_signature_clusters_host(nullptr, 3, nullptr, 32, 1, &got),
                           fdgpu_signature_clusters_host(S.data(), 65, twice.data(), 32, 1, &got), fdgpu_signature_clusters_host(S.data(), 65, beyond.data(), 32, 1, &got)};
    for (int rc : refused) bad += rc != FDGPU_EINVAL;
    bad += got != nullptr;
    puts(bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
