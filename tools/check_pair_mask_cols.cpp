// The column offsets of the MSD build's mask table (folddisco_amd/csrc/fd_pair_mask_cols.h) compiled for the host.  Reads structure lengths from
// stdin (one per line) and prints the prefix table of the batch they make, for tests/test_pair_mask_columns_host.py to compare with its own
// restatement; with --big N R it prints only the number of columns of N structures of R residues each (arithmetic only, no table), which
// passes 2^32 for N = 128, R = 65535.
//   g++ -O2 -std=c++17 -fsanitize=undefined,address -fno-sanitize-recover=undefined tools/check_pair_mask_cols.cpp -o check_pair_mask_cols
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../folddisco_amd/csrc/fd_pair_mask_cols.h"

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "--big")) {
        const uint64_t N = strtoull(argv[2], nullptr, 10), R = strtoull(argv[3], nullptr, 10);
        std::vector<uint64_t> off(N + 1);
        for (uint64_t s = 0; s <= N; ++s) off[s] = s * R;
        const uint64_t total = fd_mask_col_offsets(off.data(), N, nullptr);
        printf("total %llu per_structure %llu tiles %llu\n", (unsigned long long)total, (unsigned long long)fd_mask_cols_of_structure(R),
               (unsigned long long)(N * fd_mask_tiles(R)));
        return total == N * fd_mask_cols_of_structure(R) ? 0 : 1;
    }
    std::vector<uint64_t> off(1, 0);
    unsigned long long R;
    while (scanf("%llu", &R) == 1) off.push_back(off.back() + R);
    const uint64_t N = off.size() - 1;
    uint64_t W = 0;
    for (uint64_t s = 0; s < N; ++s) W += fd_mask_tiles(off[s + 1] - off[s]);
    std::vector<uint64_t> col(W + 1, ~0ull);
    const uint64_t total = fd_mask_col_offsets(off.data(), N, col.data());
    printf("work_items %llu total %llu\n", (unsigned long long)W, (unsigned long long)total);
    for (uint64_t w = 0; w <= W; ++w) printf("%llu\n", (unsigned long long)col[w]);
    return 0;
}
