// The encoder's rule for one element of a constant tile (folddisco_amd/csrc/fd_postings.h: fd_const_classify and its parts, fd_delta_len)
// compiled for the host against the general rule of k_index.hip on full hashes and ids: head by the 30-bit hash, delta by the
// ids, repeat by equal hash and id.  In a constant tile the element and its predecessor share the bucket and hash[23:8], so both rules see the
// key words k, pk (hash[7:0] << 24 | local id) and first_id alone.  Built with -fsanitize=undefined,address by
// tests/test_encoder_const_classify_host.py.
//   g++ -O2 -std=c++17 -fsanitize=undefined,address -fno-sanitize-recover=undefined -Itools/host_hip tools/check_enc_const.cpp -o check_enc_const
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
// the device-only helpers of fd_postings.h are not called here; they only have to parse
static inline int __ffsll(long long x) { return __builtin_ffsll(x); }
template <typename T> static inline T __shfl_up(T v, int, int) { return v; }
template <typename T> static inline T __shfl_down(T v, int, int) { return v; }
template <typename T> static inline T __shfl(T v, int, int) { return v; }
template <typename T> static inline T __shfl_xor(T v, int, int) { return v; }
#include "../folddisco_amd/csrc/fd_postings.h"

static uint64_t bad = 0, pairs = 0, lens = 0;
static uint64_t n_head = 0, n_rep = 0, n_len[6] = {0, 0, 0, 0, 0, 0}, n_rise_fall = 0, n_head_same_id = 0;

// the general rule (enc_load_classify) with the tile's bucket and u16 value
static const uint32_t BUCKET = 17, EV = 0xbeef;
static void general(uint32_t k, uint32_t pk, uint32_t first_id, bool *head, uint32_t *value, uint32_t *len) {
    const uint32_t h = BUCKET << 24 | EV << 8 | k >> 24, ph = BUCKET << 24 | EV << 8 | pk >> 24;
    const uint32_t id = first_id + (k & 0xffffffu), pid = first_id + (pk & 0xffffffu);
    *head = ph != h;
    const bool dup = !*head && pid == id;
    *value = *head ? id : id - pid;
    *len = dup ? 0u : fd_varint_len(*value);
}
static void check_pair(uint32_t pk, uint32_t k, uint32_t first_id) {      // pk <= k: the stream is sorted
    bool gh;
    uint32_t gv, gl, cv = 0, cl = 0;
    general(k, pk, first_id, &gh, &gv, &gl);
    const bool ch = fd_const_classify(k, pk, first_id, &cv, &cl);
    ++pairs;
    if (gh) ++n_head; else if (!gl) ++n_rep;
    ++n_len[gl];
    if (gh && (k & 0xffffffu) < (pk & 0xffffffu)) ++n_rise_fall;
    if (gh && (k & 0xffffffu) == (pk & 0xffffffu)) ++n_head_same_id;
    if (ch != gh || cv != gv || cl != gl) {
        if (bad++ < 10) printf("MISMATCH pk=%08x k=%08x first_id=%u: head %d/%d value %u/%u len %u/%u (const/general)\n", pk, k, first_id, ch, gh, cv, gv, cl, gl);
    }
}
static void check_len(uint32_t d) {      // d < 2^31
    ++lens;
    if (fd_delta_len(d) != (d ? fd_varint_len(d) : 0u)) {
        if (bad++ < 10) printf("MISMATCH fd_delta_len(%u) = %u, fd_varint_len %u\n", d, fd_delta_len(d), fd_varint_len(d));
    }
}

int main() {
    const uint32_t tops[] = {0u, 1u, 0x7fu, 0xfeu, 0xffu};
    const uint32_t bounds[] = {0x80u, 0x4000u, 0x200000u};      // the varint boundaries below 2^24
    const uint32_t first_ids[] = {0u, (1u << 21) - 1u, (1u << 28) - (1u << 24), (1u << 28) - 1u};
    std::vector<uint32_t> ids = {0u, 1u, 2u, (1u << 24) - 2u, (1u << 24) - 1u};
    for (uint32_t b : bounds) for (int o = -2; o <= 2; ++o) ids.push_back(b + o);
    {      // and ids a boundary value (or one beside it) apart from each of those, so that DELTAS lie at and around every boundary too
        const std::vector<uint32_t> base = ids;
        for (uint32_t a : base) for (uint32_t b : bounds) for (int o = -1; o <= 1; ++o) {
            const uint64_t x = (uint64_t)a + b + o;
            if (x < (1u << 24)) ids.push_back((uint32_t)x);
        }
        for (uint32_t a : base) ids.push_back((1u << 24) - 1u - a);      // a delta of 2^24 - 1 - a, the largest with a = 0
    }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    std::vector<uint32_t> words;
    for (uint32_t t : tops) for (uint32_t i : ids) words.push_back(t << 24 | i);
    std::sort(words.begin(), words.end());
    // every pair of neighbours pk <= k of these words: equal words (repeats), equal top bytes (deltas of every length), a rising top byte with
    // a larger, an equal and a SMALLER id (k - pk < 2^24: a head that a subtraction takes for a delta)
    for (uint32_t f : first_ids)
        for (size_t a = 0; a < words.size(); ++a)
            for (size_t b = a; b < words.size(); ++b) check_pair(words[a], words[b], f);
    check_pair(0x01000005u, 0x02000001u, 0u);      // the example of fd_postings.h
    uint64_t x = 0x9e3779b97f4a7c15ull;      // xorshift64*
    for (uint32_t r = 0; r < (1u << 20); ++r) {
        x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
        const uint64_t q = x * 0x2545f4914f6cdd1dull;
        uint32_t pk = (uint32_t)(q >> 32), k = (uint32_t)q;
        if (r & 1u) k = (pk & 0xff000000u) | (k & 0xffffffu);      // every second pair inside one list
        if (k < pk) std::swap(k, pk);
        check_pair(pk, k, first_ids[r & 3u]);
        check_len((uint32_t)(q >> 33) >> (uint32_t)(q & 31u));
    }
    for (uint32_t d = 0; d < (1u << 24); ++d) check_len(d);      // every delta a constant tile can hold
    for (uint64_t p = 1; p < (1ull << 31); p *= 2) { check_len((uint32_t)(p - 1)); check_len((uint32_t)p); check_len((uint32_t)(p + 1 < (1ull << 31) ? p + 1 : p)); }
    // the cases must be there
    const bool covered = n_head > 1000 && n_rep > 100 && n_len[1] && n_len[2] && n_len[3] && n_len[4] && n_len[5] && n_rise_fall > 1000 && n_head_same_id > 100;
    if (!covered) { printf("MISMATCH coverage: heads %llu repeats %llu rise-and-fall %llu\n", (unsigned long long)n_head, (unsigned long long)n_rep, (unsigned long long)n_rise_fall); ++bad; }
    printf("checked %llu pairs (%llu heads, %llu with a smaller id, %llu repeats), %llu lengths, mismatches: %llu\n", (unsigned long long)pairs,
           (unsigned long long)n_head, (unsigned long long)n_rise_fall, (unsigned long long)n_rep, (unsigned long long)lens, (unsigned long long)bad);
    return bad ? 1 : 0;
}
