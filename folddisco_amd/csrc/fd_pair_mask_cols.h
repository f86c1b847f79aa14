// fd_pair_mask_cols.h — where the pass masks of a work item lie in the MSD build's mask table (k_hash.hip: k_pair_count_msd writes them,
// k_pair_emit2<.., MASKS> replays them).  Host-compilable: no HIP type, tools/check_pair_mask_cols.cpp calls it without a device.
//
// A work item is one 64-residue i-tile of a structure, first residue i0, and meets the partners j = i0 .. r1 - 1 (r1: the structure's end):
// r1 - i0 COLUMNS, one u64 each (bit l: lane l of the tile emits the pair (i0 + l, j)).  The kernels walk the partners in blocks of 64 and the
// count pass stores a block's 64 words with one 8-byte store per lane, so a work item's columns are padded to whole blocks — every word it writes
// is the work item's own, no kernel needs a bound inside a block, and the padding is written (as zeros) like every other column.  The offsets are 64-bit: a call of 2^24 structures holds ~2.2e10 columns.
#pragma once
#include <stdint.h>

#define FD_MASK_BLOCK 64ull      // columns per block = partners per block = FD_WAVE
#define FD_MASK_SLACK_WORDS 8ull // allocated behind the last column: the replay takes two words at a time, also at column 63 of the last block

// columns a work item owns in the table, `partners` = r1 - i0 >= 1
static inline uint64_t fd_mask_cols_padded(uint64_t partners) { return (partners + (FD_MASK_BLOCK - 1)) / FD_MASK_BLOCK * FD_MASK_BLOCK; }

// work items of a structure of R residues (one per 64-residue tile; none for an empty structure)
static inline uint64_t fd_mask_tiles(uint64_t R) { return (R + (FD_MASK_BLOCK - 1)) / FD_MASK_BLOCK; }

// columns of all work items of a structure of R residues: tile t meets R - 64 t partners
static inline uint64_t fd_mask_cols_of_structure(uint64_t R) {
    uint64_t n = 0;
    for (uint64_t t = 0; t < R; t += FD_MASK_BLOCK) n += fd_mask_cols_padded(R - t);
    return n;
}

// The prefix table of a batch: wi_col[w] = first column of work item w, wi_col[n_work] = columns of the table; work items in the order of
// fd_build_work_items (structure by structure, tile by tile).  res_off: [n_struct + 1] residue offsets.  wi_col may be null (the total alone).
// Returns the number of columns.
static inline uint64_t fd_mask_col_offsets(const uint64_t *res_off, uint64_t n_struct, uint64_t *wi_col) {
    uint64_t col = 0, w = 0;
    for (uint64_t s = 0; s < n_struct; ++s) {
        const uint64_t R = res_off[s + 1] - res_off[s];
        for (uint64_t t = 0; t < R; t += FD_MASK_BLOCK) {
            if (wi_col) wi_col[w] = col;
            ++w;
            col += fd_mask_cols_padded(R - t);
        }
    }
    if (wi_col) wi_col[w] = col;
    return col;
}
