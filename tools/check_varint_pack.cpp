// fd_varint_pack (folddisco_amd/csrc/fd_postings.h) compiled for the host against the byte-wise writer fd_put_varint: every v below 2^22,
// every power of 128 and its two neighbours, 2^32 - 1 and 2^24 random values; the bytes above the varint must be zero and len = 0 with v = 0
// must give 0.  Built with -fsanitize=undefined by tests/test_varint_pack_host.py: a shift by the operand's width shows up as a report.
//   g++ -O2 -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined -Itools/host_hip tools/check_varint_pack.cpp -o check_varint_pack
#include <stdint.h>
#include <stdio.h>
#include <string.h>
// the device-only helpers of fd_postings.h are not called here; they only have to parse
static inline int __ffsll(long long x) { return __builtin_ffsll(x); }
template <typename T> static inline T __shfl_up(T v, int, int) { return v; }
template <typename T> static inline T __shfl_down(T v, int, int) { return v; }
template <typename T> static inline T __shfl(T v, int, int) { return v; }
template <typename T> static inline T __shfl_xor(T v, int, int) { return v; }
#include "../folddisco_amd/csrc/fd_postings.h"

static uint64_t bad = 0, checked = 0;
static void check(uint32_t v) {
    uint8_t ref[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned n = fd_put_varint(v, ref);
    const uint32_t len = fd_varint_len(v);
    uint64_t want;
    memcpy(&want, ref, 8);      // little endian: byte k of the varint is bits 8k .. 8k + 7
    const uint64_t got = fd_varint_pack(v, len);
    ++checked;
    if (n != len || got != want || (len < 8 && (got >> (8 * len)) != 0)) {
        if (bad++ < 10) printf("MISMATCH v=%u len=%u (writer %u) pack=%016llx want=%016llx\n", v, len, n, (unsigned long long)got, (unsigned long long)want);
    }
}

int main() {
    for (uint32_t v = 0; v < (1u << 22); ++v) check(v);
    for (uint64_t p = 1; p <= 0xffffffffull; p *= 128) { check((uint32_t)(p - 1)); check((uint32_t)p); check((uint32_t)(p + 1)); }
    check(0xffffffffu); check(0xfffffffeu); check(0x80000000u);
    uint64_t x = 0x9e3779b97f4a7c15ull;      // xorshift64*: top 32 bits, shifted down by 0..31 so that every length is drawn often
    for (uint32_t k = 0; k < (1u << 24); ++k) {
        x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
        const uint64_t r = x * 0x2545f4914f6cdd1dull;
        check((uint32_t)(r >> 32) >> (uint32_t)(r & 31u));
    }
    if (fd_varint_pack(0u, 0u) != 0) { printf("MISMATCH pack(0, 0) != 0\n"); ++bad; }
    printf("checked %llu values, mismatches: %llu\n", (unsigned long long)checked, (unsigned long long)bad);
    return bad ? 1 : 0;
}
