// hulk_links_place.h — where an edge of hulk_links goes (hulk_links.hip): the arithmetic between the masks of k_links_count and the
// slots k_links_fill writes.  HIP-free: the including file defines
//   HULK_LP_FN               the function qualifiers (__device__ __forceinline__ / static inline)
// so tests/cpp/links_place_host.cpp compiles this very text for the host and restates the three kernels around it.
//
// A MASK is the 64 compares of one subject row against one tile of 64 other columns: bit b set = column 64 * tile + b is an edge of
// the row.  A thread of the pair tile (hulk_pairtile.h) owns columns 4 * tx .. 4 * tx + 3 of four rows: its four compares of a row
// are the nibble at bit 4 * tx of that row's mask (links_quad_word).  Ascending bits are ascending columns, ascending tiles are
// ascending columns too, so
//   slot(row, tile, bit) = row_start[row] + offset[row][tile] + popcount(mask[row][tile] & links_below(bit))
// with offset[row][.] the exclusive scan of the popcounts along the row (links_advance, tile by tile) and row_start the exclusive scan
// of the row totals, numbers the edges of a row in ascending column order, the rows one behind the other, and hits every slot below
// the grand total exactly once: the layout is a function of the masks alone.  A row's degree is below 2^32 (n is); the totals
// are 64-bit.
#ifndef HULK_LINKS_PLACE_H
#define HULK_LINKS_PLACE_H

#include <stdint.h>

HULK_LP_FN uint32_t links_popc(uint64_t mask) { return (uint32_t)__builtin_popcountll(mask); }

// the bits of the columns in front of column `bit` of the tile (bit < 64)
HULK_LP_FN uint64_t links_below(uint32_t bit) { return (1ull << bit) - 1ull; }

// the four compares of the thread with other-quad tx (bit j: column 4 * tx + j), in their place in the row's mask
HULK_LP_FN uint64_t links_quad_word(uint32_t nibble, uint32_t tx) { return (uint64_t)(nibble & 15u) << (4u * tx); }
HULK_LP_FN uint32_t links_quad_of(uint64_t mask, uint32_t tx) { return (uint32_t)(mask >> (4u * tx)) & 15u; }

// one step along a row: the offset of this tile's edges inside the row; `running` moves behind them
HULK_LP_FN uint32_t links_advance(uint64_t mask, uint32_t *running) {
    const uint32_t at = *running;
    *running = at + links_popc(mask);
    return at;
}

// the slot of the edge at column `bit` of a tile (the bit is set in mask)
HULK_LP_FN uint64_t links_slot(uint64_t row_start, uint32_t tile_offset, uint64_t mask, uint32_t bit) {
    return row_start + tile_offset + links_popc(mask & links_below(bit));
}

#endif
