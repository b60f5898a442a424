// hulk_amd/csrc/hulk_links_place.h compiled for the host (it is HIP-free), under -fsanitize=address,undefined, with the three kernels
// of hulk_links.hip restated around it the way they use it: the masks [tile][row] of a band; k_links_rows' 16 segments of the tile range
// (popcounts, the exclusive scan over the segments, the offsets); k_links_scan's exclusive scan of the degrees; k_links_fill's slot of
// every set bit, thread by thread (16 other-quads x 4 columns).  Checked: the slots of a band are hit exactly once, none outside
// [0, total), and every row's slots hold its columns in ascending order — against a plain enumeration of the set bits.
//   links_place_host          prints one "<case>: ok" line per case, "FAILED ..." and exit 1 otherwise
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#define HULK_LP_FN static inline
#include "hulk_links_place.h"

static const int SEGS = 16;

static bool run_case(const std::string &name, uint32_t rows, uint32_t qt0, uint32_t NT, const std::vector<uint64_t> &mask /* [NT][rows] */) {
    auto at = [&](uint32_t t, uint32_t r) { return (size_t)t * rows + r; };
    // k_links_rows
    std::vector<uint32_t> offset((size_t)NT * rows, 0xdeadbeefu), degree(rows, 0);
    const uint32_t per = (NT - qt0 + SEGS - 1) / SEGS;
    for (uint32_t r = 0; r < rows; r++) {
        uint32_t seg_count[SEGS];
        for (uint32_t y = 0; y < (uint32_t)SEGS; y++) {
            const uint32_t ta = qt0 + y * per < NT ? qt0 + y * per : NT, tb = ta + per < NT ? ta + per : NT;
            uint32_t running = 0;
            for (uint32_t t = ta; t < tb; t++) links_advance(mask[at(t, r)], &running);
            seg_count[y] = running;
        }
        for (uint32_t y = 0; y < (uint32_t)SEGS; y++) {
            const uint32_t ta = qt0 + y * per < NT ? qt0 + y * per : NT, tb = ta + per < NT ? ta + per : NT;
            uint32_t running = 0;
            for (uint32_t z = 0; z < y; z++) running += seg_count[z];
            for (uint32_t t = ta; t < tb; t++) offset[at(t, r)] = links_advance(mask[at(t, r)], &running);
            if (y == (uint32_t)SEGS - 1) degree[r] = running;
        }
    }
    // k_links_scan
    std::vector<uint64_t> row_start(rows);
    uint64_t total = 0;
    for (uint32_t r = 0; r < rows; r++) { row_start[r] = total; total += degree[r]; }
    // the plain enumeration
    std::vector<uint32_t> want;
    std::vector<uint64_t> want_start(rows);
    for (uint32_t r = 0; r < rows; r++) {
        want_start[r] = want.size();
        for (uint32_t t = qt0; t < NT; t++)
            for (uint32_t b = 0; b < 64; b++) if ((mask[at(t, r)] >> b) & 1) want.push_back(64 * t + b);
    }
    if (want.size() != total) { printf("FAILED %s: total %llu, want %zu\n", name.c_str(), (unsigned long long)total, want.size()); return false; }
    for (uint32_t r = 0; r < rows; r++)
        if (row_start[r] != want_start[r]) { printf("FAILED %s: row_start[%u] %llu, want %llu\n", name.c_str(), r, (unsigned long long)row_start[r], (unsigned long long)want_start[r]); return false; }
    // k_links_fill, in an order that is not the rows': tiles descending, threads descending
    std::vector<uint32_t> col(total, 0), hits(total, 0);
    for (uint32_t t = NT; t-- > qt0;)
        for (uint32_t r = rows; r-- > 0;) {
            const uint64_t m = mask[at(t, r)];
            for (uint32_t tx = 16; tx-- > 0;) {
                if (!links_quad_of(m, tx)) continue;
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t bit = 4 * tx + j;
                    if (!((m >> bit) & 1)) continue;
                    const uint64_t slot = links_slot(row_start[r], offset[at(t, r)], m, bit);
                    if (slot >= total) { printf("FAILED %s: slot %llu outside %llu\n", name.c_str(), (unsigned long long)slot, (unsigned long long)total); return false; }
                    hits[slot]++; col[slot] = 64 * t + bit;
                }
            }
        }
    for (uint64_t e = 0; e < total; e++) {
        if (hits[e] != 1) { printf("FAILED %s: slot %llu written %u times\n", name.c_str(), (unsigned long long)e, hits[e]); return false; }
        if (col[e] != want[e]) { printf("FAILED %s: slot %llu holds column %u, want %u\n", name.c_str(), (unsigned long long)e, col[e], want[e]); return false; }
    }
    for (uint32_t r = 0; r < rows; r++)
        for (uint64_t e = row_start[r] + 1; e < row_start[r] + degree[r]; e++)
            if (col[e - 1] >= col[e]) { printf("FAILED %s: row %u is not ascending\n", name.c_str(), r); return false; }
    printf("%s: ok (%llu edges)\n", name.c_str(), (unsigned long long)total);
    return true;
}

int main() {
    bool ok = true;
    // the count epilogue's combine: the nibbles of the 16 other-quads of a row are its mask
    {
        std::mt19937_64 rng(5);
        for (int rep = 0; rep < 1000 && ok; rep++) {
            const uint64_t m = rep == 0 ? 0 : rep == 1 ? ~0ull : rng();
            uint64_t word = 0;
            for (uint32_t tx = 0; tx < 16; tx++) word |= links_quad_word(links_quad_of(m, tx), tx);
            if (word != m) { printf("FAILED quads: %llx from %llx\n", (unsigned long long)word, (unsigned long long)m); ok = false; }
        }
        if (links_below(0) != 0 || links_below(63) != 0x7fffffffffffffffull || links_popc(~0ull) != 64 || links_popc(0) != 0) { printf("FAILED below / popc\n"); ok = false; }
        if (ok) printf("quads: ok\n");
    }
    const uint32_t shapes[][3] = {{32, 0, 1}, {32, 0, 5}, {96, 0, 17}, {64, 3, 17}, {33, 0, 40}, {64, 39, 40}, {7, 2, 300}};   // rows, qt0, NT
    std::mt19937_64 rng(11);
    for (const auto &sh : shapes) {
        const uint32_t rows = sh[0], qt0 = sh[1], NT = sh[2];
        const std::string tag = " rows " + std::to_string(rows) + " tiles " + std::to_string(qt0) + ".." + std::to_string(NT);
        const size_t cells = (size_t)NT * rows;
        // (the tiles in front of qt0 hold garbage: nobody reads them)
        auto fresh = [&](uint64_t fill) { std::vector<uint64_t> m(cells, fill); for (uint32_t t = 0; t < qt0; t++) for (uint32_t r = 0; r < rows; r++) m[(size_t)t * rows + r] = 0xa5a5a5a5a5a5a5a5ull; return m; };
        ok = run_case("all zeros" + tag, rows, qt0, NT, fresh(0)) && ok;
        ok = run_case("all ones" + tag, rows, qt0, NT, fresh(~0ull)) && ok;
        { auto m = fresh(0); m[(size_t)qt0 * rows + 0] = 1; ok = run_case("the first bit" + tag, rows, qt0, NT, m) && ok; }
        { auto m = fresh(0); m[(size_t)(NT - 1) * rows + rows - 1] = 1ull << 63; ok = run_case("the last bit" + tag, rows, qt0, NT, m) && ok; }
        { auto m = fresh(0); for (uint32_t r = 0; r < rows; r++) { m[(size_t)qt0 * rows + r] = 1; m[(size_t)(NT - 1) * rows + r] |= 1ull << 63; } ok = run_case("both ends of every row" + tag, rows, qt0, NT, m) && ok; }
        for (const int density : {1, 8, 32, 63}) {
            auto m = fresh(0);
            for (uint32_t t = qt0; t < NT; t++)
                for (uint32_t r = 0; r < rows; r++) {
                    uint64_t w = 0;
                    for (int b = 0; b < 64; b++) if ((int)(rng() % 64) < density) w |= 1ull << b;
                    if (density == 1 && rng() % 4) w = 0;           // (mostly empty tiles)
                    m[(size_t)t * rows + r] = w;
                }
            ok = run_case("random " + std::to_string(density) + "/64" + tag, rows, qt0, NT, m) && ok;
        }
    }
    return ok ? 0 : 1;
}
