// fd_signatures_host.cpp — fdgpu_signatures_host and fdgpu_signature_pairs_host: the index signatures (k_sig.hip) and their compare on host
// arrays.  No device and no HIP call: this file also builds with a plain host compiler.
//
// Signatures, on purpose by another algorithm than the device's (which transposes the window and reduces every row): ONE pass over the posting
// lists, m(h) once per list, and every decoded id of the range updates its record in place (n += 1, d0 += m, d1 ^= m, sk[b] = min).  Threads
// split the structure range and each walks all lists, so no two threads touch the same record and the result does not depend on their number.
// Every thread makes the checks of fdgpu_rows_host on every list (the same lists are left behind their head: those that start at or above id_hi),
// so the same input gives the same error code; nothing is handed out unless every list was sound.
// Pairs: a blocked double loop, threads over the blocks of A, the records sorted by (a, b) at the end.
// Neighbours: the same blocked loop over (Q blocks x D blocks), threads over the Q blocks; every query's k-list is its row of the result, kept
// sorted by insertion under fd_sig_nearer, so no two threads touch the same row and the result does not depend on their number.
// Clusters: the sequential walk in blocks of 1024 positions.  Per block, threads over its positions find each one's nearest among the
// representatives chosen BEFORE the block (a position belongs to one thread: nothing depends on their number); then the block is settled in walk
// order on the calling thread: a position without a best becomes a representative and every later position of the block that qualifies with it
// and finds it nearer takes it.
#include <cstring>
#include "fd_signature.h"
#include "fd_postings_host.h"

namespace {
struct sg_in { const uint32_t *hashes; const uint64_t *offsets; const uint8_t *value; uint64_t value_len, first_id, S, lo, hi; };

// list k walked for the thread that owns the structures s0 .. s1 - 1 (absolute ids); error bits as rows_list: 1 damaged, 2 a list of 4 GiB
unsigned sig_list(const sg_in &A, uint64_t k, uint64_t s0, uint64_t s1, fd_signature *tab) {
    const uint64_t b0 = A.offsets[k], b1 = A.offsets[k + 1];
    if (b1 <= b0 || b1 > A.value_len) return 1u;
    if (b1 - b0 > 0xffffffffull) return 2u;
    if (A.value[b1 - 1] & 0x80) return 1u;
    const uint64_t m = fd_sig_mix(A.hashes[k]);
    const uint32_t b = fd_sig_bucket(m), v = fd_sig_value(m);
    uint64_t run = 0;
    for (uint64_t q = b0; q < b1;) {
        const fd_varint_read vr = fd_read_varint(A.value, q, b1);
        if (vr.st != FD_VR_OK) return 1u;
        run += vr.v;                               // the head is absolute: 0 + head
        if (run < A.first_id || run - A.first_id >= A.S) return 1u;
        if (q == b0 && run >= A.hi) break;
        if (run >= s0 && run < s1) {
            fd_signature &g = tab[run - A.lo];
            g.n += 1; g.d0 += m; g.d1 ^= m;
            if (v < g.sk[b]) g.sk[b] = v;
        }
        q += vr.n;
    }
    return 0;
}

struct sg_stat { uint32_t eq, E; };
inline sg_stat sig_compare(const fd_signature &a, const fd_signature &b) {
    sg_stat s = {0, 0};
    for (unsigned k = 0; k < 64; ++k) {
        s.eq += a.sk[k] == b.sk[k] ? 1u : 0u;
        s.E += (a.sk[k] == FD_SIG_EMPTY && b.sk[k] == FD_SIG_EMPTY) ? 1u : 0u;
    }
    return s;
}
}      // namespace

extern "C" int fdgpu_signatures_host(const uint32_t *hashes, const uint64_t *offsets, uint64_t H, const uint8_t *value, uint64_t value_len, uint64_t first_id,
                                     uint64_t n_structures, uint64_t id_lo, uint64_t id_hi, uint32_t n_threads, fd_signature **out) {
    if (!out) return FDGPU_EINVAL;
    *out = nullptr;
    if ((H && (!offsets || !hashes)) || (value_len && !value)) return FDGPU_EINVAL;
    if (first_id > 0xffffffffull || first_id + n_structures > 0xffffffffull) return FDGPU_EINVAL;
    if (id_lo < first_id || id_lo > id_hi || id_hi > first_id + n_structures) return FDGPU_EINVAL;
    const uint64_t W = id_hi - id_lo;
    fd_signature *tab = (fd_signature *)malloc(std::max<uint64_t>(W, 1) * sizeof(fd_signature));
    if (!tab) return FDGPU_ENOMEM;
    for (uint64_t s = 0; s < W; ++s) {
        memset(&tab[s], 0, 24);
        for (unsigned k = 0; k < 64; ++k) tab[s].sk[k] = FD_SIG_EMPTY;
    }
    if (W && H) {
        const sg_in A{hashes, offsets, value, value_len, first_id, n_structures, id_lo, id_hi};
        const uint64_t T = fd_host_threads(n_threads, W, 64);
        std::vector<unsigned> err(T, 0);
        fd_over_ranges(T, [&](uint64_t t) {
            const uint64_t s0 = id_lo + W * t / T, s1 = id_lo + W * (t + 1) / T;
            for (uint64_t k = 0; k < H; ++k) err[t] |= sig_list(A, k, s0, s1, tab);
        });
        unsigned eb = 0;
        for (unsigned e : err) eb |= e;
        if (eb) { free(tab); return eb & 1u ? FDGPU_EINVAL : FDGPU_ERANGE; }
    }
    *out = tab;
    return FDGPU_OK;
}

extern "C" int fdgpu_signature_pairs_host(const fd_signature *A, uint64_t nA, const fd_signature *B, uint64_t nB, uint32_t thr64, uint64_t max_pairs,
                                          uint32_t n_threads, fd_sig_pair **pairs, uint64_t *n_pairs) {
    if (!pairs || !n_pairs) return FDGPU_EINVAL;
    *pairs = nullptr; *n_pairs = 0;
    if (thr64 < 1 || thr64 > 64) return FDGPU_EINVAL;
    if (nA > 0xffffffffull || (B && nB > 0xffffffffull) || (nA && !A)) return FDGPU_EINVAL;
    const bool self = B == nullptr;
    if (self) { B = A; nB = nA; }
    const uint64_t BLK = 64, n_blk = (nA + BLK - 1) / BLK;
    const uint64_t T = fd_host_threads(n_threads, n_blk, 1);
    std::vector<std::vector<fd_sig_pair>> got(T);
    std::vector<uint64_t> cnt(T, 0);
    bool oom = false;
    fd_over_ranges(T, [&](uint64_t t) {
        try {
            for (uint64_t ba = n_blk * t / T; ba < n_blk * (t + 1) / T; ++ba) {
                const uint64_t a0 = ba * BLK, a1 = std::min(nA, a0 + BLK);
                for (uint64_t b0 = self ? a0 : 0; b0 < nB; b0 += BLK) {      // self mode: the blocks below the diagonal hold no a < b
                    const uint64_t b1 = std::min(nB, b0 + BLK);
                    for (uint64_t a = a0; a < a1; ++a) {
                        if (!A[a].n) continue;
                        for (uint64_t b = self ? std::max(b0, a + 1) : b0; b < b1; ++b) {
                            const sg_stat s = sig_compare(A[a], B[b]);
                            if (!fd_sig_reported(A[a].n, B[b].n, s.eq, s.E, thr64)) continue;
                            if (++cnt[t] > max_pairs) continue;               // counted, not kept: the call ends with the true count
                            fd_sig_pair r;
                            r.a = (uint32_t)a; r.b = (uint32_t)b; r.match = (uint8_t)(s.eq - s.E); r.filled = (uint8_t)(64u - s.E);
                            r.flags = A[a].n == B[b].n && A[a].d0 == B[b].d0 && A[a].d1 == B[b].d1 ? FD_SIG_IDENTICAL : 0u;
                            got[t].push_back(r);
                        }
                    }
                }
            }
        } catch (...) { oom = true; }
    });
    if (oom) return FDGPU_ENOMEM;
    uint64_t total = 0;
    for (uint64_t x : cnt) total += x;
    *n_pairs = total;
    if (total > max_pairs) return FDGPU_ERANGE;
    fd_sig_pair *res = (fd_sig_pair *)malloc(std::max<uint64_t>(total, 1) * sizeof(fd_sig_pair));
    if (!res) return FDGPU_ENOMEM;
    uint64_t at = 0;
    for (auto &g : got) { if (!g.empty()) memcpy(res + at, g.data(), g.size() * sizeof(fd_sig_pair)); at += g.size(); }
    std::sort(res, res + total, [](const fd_sig_pair &x, const fd_sig_pair &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    *pairs = res;
    return FDGPU_OK;
}

extern "C" int fdgpu_signature_neighbors_host(const fd_signature *Q, uint64_t nQ, const fd_signature *D, uint64_t nD, const uint32_t *exclude, uint32_t k,
                                              uint32_t thr64, uint32_t n_threads, fd_sig_neighbor **out) {
    if (!out) return FDGPU_EINVAL;
    *out = nullptr;
    if (k < 1 || k > FD_SIG_MAX_K || thr64 < 1 || thr64 > 64) return FDGPU_EINVAL;
    if (nQ > 0xffffffffull || (D && nD > 0xffffffffull) || (nQ && !Q) || (!D && exclude)) return FDGPU_EINVAL;
    const bool self = D == nullptr;
    if (self) { D = Q; nD = nQ; }
    fd_sig_neighbor *res = (fd_sig_neighbor *)malloc(std::max<uint64_t>(nQ * k, 1) * sizeof(fd_sig_neighbor));
    if (!res) return FDGPU_ENOMEM;
    const fd_sig_neighbor none = {FD_SIG_NO_ID, 0, 0, 0};
    for (uint64_t i = 0; i < std::max<uint64_t>(nQ * k, 1); ++i) res[i] = none;
    const uint64_t BLK = 64, n_blk = (nQ + BLK - 1) / BLK;
    const uint64_t T = fd_host_threads(n_threads, n_blk, 1);
    fd_over_ranges(T, [&](uint64_t t) {
        for (uint64_t bq = n_blk * t / T; bq < n_blk * (t + 1) / T; ++bq) {
            const uint64_t q0 = bq * BLK, q1 = std::min(nQ, q0 + BLK);
            for (uint64_t d0 = 0; d0 < nD; d0 += BLK) {
                const uint64_t d1 = std::min(nD, d0 + BLK);
                for (uint64_t q = q0; q < q1; ++q) {
                    if (!Q[q].n) continue;
                    const uint64_t skip = self ? q : exclude ? exclude[q] : FD_SIG_NO_ID;
                    fd_sig_neighbor *row = res + q * k;
                    for (uint64_t d = d0; d < d1; ++d) {
                        if (d == skip) continue;
                        const sg_stat s = sig_compare(Q[q], D[d]);
                        if (!fd_sig_reported(Q[q].n, D[d].n, s.eq, s.E, thr64)) continue;
                        const uint32_t m = s.eq - s.E, f = 64u - s.E;
                        uint32_t at = k;                                      // the slot it takes: behind everything that is nearer
                        while (at > 0 && fd_sig_nearer(m, f, (uint32_t)d, row[at - 1].match, row[at - 1].filled, row[at - 1].id)) --at;
                        if (at == k) continue;
                        for (uint32_t j = k - 1; j > at; --j) row[j] = row[j - 1];
                        row[at].id = (uint32_t)d; row[at].match = (uint8_t)m; row[at].filled = (uint8_t)f;
                        row[at].flags = Q[q].n == D[d].n && Q[q].d0 == D[d].d0 && Q[q].d1 == D[d].d1 ? FD_SIG_IDENTICAL : 0u;
                    }
                }
            }
        }
    });
    *out = res;
    return FDGPU_OK;
}

uint64_t fd_sig_order_fault(const uint32_t *order, uint64_t n) {
    try {
        std::vector<uint64_t> seen((n + 63) / 64, 0);
        for (uint64_t w = 0; w < n; ++w) {
            const uint64_t p = order[w];
            if (p >= n || (seen[p >> 6] >> (p & 63) & 1u)) return w;
            seen[p >> 6] |= 1ull << (p & 63);
        }
    } catch (...) { return FD_SIG_ORDER_NOMEM; }
    return n;
}

// both host forms of the clusters.  During the walk res[p].id is a combined id (seed j: j, position r of S: nT + r), which is the order
// the definition asks for; the ids are turned back at the end.  nT == 0: the unseeded walk, where the two coincide
static int clusters_host(const fd_signature *S, uint64_t n, const uint32_t *order, const fd_signature *T, uint64_t nT, uint32_t thr64, uint32_t n_threads,
                         fd_sig_neighbor **out) {
    if (!out) return FDGPU_EINVAL;
    *out = nullptr;
    if (thr64 < 1 || thr64 > 64 || n > 0xffffffffull || (n && !S)) return FDGPU_EINVAL;
    if ((nT && !T) || nT > 0xffffffffull || nT + n > 0xffffffffull) return FDGPU_EINVAL;
    if (order) {
        const uint64_t w = fd_sig_order_fault(order, n);
        if (w != n) return w == FD_SIG_ORDER_NOMEM ? FDGPU_ENOMEM : FDGPU_EINVAL;
    }
    fd_sig_neighbor *res = (fd_sig_neighbor *)malloc(std::max<uint64_t>(n, 1) * sizeof(fd_sig_neighbor));
    if (!res) return FDGPU_ENOMEM;
    const fd_sig_neighbor none = {FD_SIG_NO_ID, 0, 0, 0};
    for (uint64_t i = 0; i < std::max<uint64_t>(n, 1); ++i) res[i] = none;
    auto take = [&](uint64_t p, const fd_signature &r, uint64_t id) {     // r, a representative with that combined id, for p if the pair is reported and r is nearer than p's best
        const sg_stat s = sig_compare(S[p], r);
        if (!fd_sig_reported(S[p].n, r.n, s.eq, s.E, thr64)) return;
        const uint32_t m = s.eq - s.E, f = 64u - s.E;
        fd_sig_neighbor &b = res[p];
        if (!fd_sig_nearer(m, f, (uint32_t)id, b.match, b.filled, b.id)) return;
        b.id = (uint32_t)id; b.match = (uint8_t)m; b.filled = (uint8_t)f;
        b.flags = S[p].n == r.n && S[p].d0 == r.d0 && S[p].d1 == r.d1 ? FD_SIG_IDENTICAL : 0u;
    };
    if (nT) {                                           // every position's nearest seed: the seeds do not change during the walk
        const uint64_t BLK = 64, n_blk = (n + BLK - 1) / BLK;
        const uint64_t TH = fd_host_threads(n_threads, n_blk, 1);
        fd_over_ranges(TH, [&](uint64_t t) {
            for (uint64_t bp = n_blk * t / TH; bp < n_blk * (t + 1) / TH; ++bp)
                for (uint64_t j0 = 0; j0 < nT; j0 += BLK)
                    for (uint64_t p = bp * BLK; p < std::min(n, bp * BLK + BLK); ++p) {
                        if (!S[p].n) continue;
                        for (uint64_t j = j0; j < std::min(nT, j0 + BLK); ++j) take(p, T[j], j);
                    }
        });
    }
    std::vector<uint32_t> reps;
    const uint64_t BLK = 1024;
    try {
        for (uint64_t w0 = 0; w0 < n; w0 += BLK) {
            const uint64_t nb = std::min(BLK, n - w0), R = reps.size();
            auto at = [&](uint64_t i) { return order ? (uint64_t)order[w0 + i] : w0 + i; };
            const uint64_t TH = fd_host_threads(n_threads, nb * R, 1u << 16);     // a thread is worth starting for 65,536 compares
            fd_over_ranges(TH, [&](uint64_t t) {
                for (uint64_t i = nb * t / TH; i < nb * (t + 1) / TH; ++i) {
                    const uint64_t p = at(i);
                    if (!S[p].n) continue;
                    for (uint64_t k = 0; k < R; ++k) take(p, S[reps[k]], nT + reps[k]);
                }
            });
            for (uint64_t i = 0; i < nb; ++i) {
                const uint64_t p = at(i);
                if (!S[p].n || res[p].id != FD_SIG_NO_ID) continue;
                uint32_t filled = 0;
                for (unsigned k = 0; k < 64; ++k) filled += S[p].sk[k] != FD_SIG_EMPTY ? 1u : 0u;
                res[p].id = (uint32_t)(nT + p); res[p].match = res[p].filled = (uint8_t)filled; res[p].flags = FD_SIG_IDENTICAL;
                reps.push_back((uint32_t)p);
                for (uint64_t j = i + 1; j < nb; ++j) if (S[at(j)].n) take(at(j), S[p], nT + p);
            }
        }
    } catch (...) { free(res); return FDGPU_ENOMEM; }
    for (uint64_t p = 0; nT && p < n; ++p) {
        fd_sig_neighbor &b = res[p];
        if (b.id == FD_SIG_NO_ID) continue;
        if (b.id < nT) b.flags |= FD_SIG_SEED; else b.id -= (uint32_t)nT;
    }
    *out = res;
    return FDGPU_OK;
}

extern "C" int fdgpu_signature_clusters_host(const fd_signature *S, uint64_t n, const uint32_t *order, uint32_t thr64, uint32_t n_threads,
                                             fd_sig_neighbor **out) {
    return clusters_host(S, n, order, nullptr, 0, thr64, n_threads, out);
}

extern "C" int fdgpu_signature_clusters_seeded_host(const fd_signature *S, uint64_t n, const uint32_t *order, const fd_signature *T, uint64_t nT,
                                                    uint32_t thr64, uint32_t n_threads, fd_sig_neighbor **out) {
    return clusters_host(S, n, order, T, nT, thr64, n_threads, out);
}
