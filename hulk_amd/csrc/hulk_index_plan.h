// hulk_index_plan.h — how hulk_index_search (hulk_index.hip) cuts its work into launches.  HIP-free: tests/cpp/index_plan_host.cpp runs
// this text on the host at the sizes no test can allocate on a device.
// The HIP runtime refuses a launch of 2^32 threads or more in x.  k_index_probe gives a wave (64 threads) to every (query, band) of a
// launch and k_index_verify one to every candidate of a block, so neither may be handed more than INDEX_MAX_WAVES items at once:
//   the count pass   runs over chunks of index_count_chunk(B) queries
//   a block          holds at most that many queries and at most min(scratch_bytes / INDEX_CAND_BYTES, INDEX_MAX_WAVES) candidates
//   what is left     k_index_keys and the sort's first kernel run a thread per (sketch, band): n B and m B stay below 2^32
//                    (index_threads_ok; refused before any HIP call)
// A block is a run of consecutive queries whose candidates fit together; a single query above the cap goes alone, in pieces of `cap`
// candidates [lo, lo + count) of its own numbering.  Blocks and pieces only window one numbering: they cannot change a result.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace hulk {

constexpr uint64_t INDEX_CAND_BYTES = 16;                          // a candidate in the scratch: sketch, query, distance
constexpr uint32_t INDEX_MAX_BANDS = 65535;                        // (grid.y of the sort)
constexpr uint32_t INDEX_MAX_WAVES = 1u << 25;                     // waves of one launch: 2^31 threads

inline bool index_threads_ok(uint64_t sketches, uint32_t B) { return sketches * B < (1ull << 32); }

// queries a launch of k_index_probe takes: at least 512 (B <= INDEX_MAX_BANDS)
inline uint32_t index_count_chunk(uint32_t B) { return INDEX_MAX_WAVES / B; }

// candidates a block holds
inline uint32_t index_block_cap(uint64_t scratch_bytes) { return (uint32_t)std::min<uint64_t>(scratch_bytes / INDEX_CAND_BYTES, INDEX_MAX_WAVES); }

struct IndexBlock { uint32_t q0, nq, lo, count; };                 // queries [q0, q0 + nq); nq == 1: the candidates [lo, lo + count) of q0

struct IndexPlan {
    std::vector<IndexBlock> blocks;                                // (a run of queries without any candidate makes no block)
    uint32_t query_blocks = 0, pieces = 0, longest = 0, biggest = 0;   // longest: the most queries, biggest: the most candidates of a block
};

// tot[q], q < m: the candidates of query q; cap >= 1
inline IndexPlan index_plan(const uint32_t *tot, uint32_t m, uint32_t B, uint32_t cap) {
    IndexPlan p;
    const uint32_t most = index_count_chunk(B);
    for (uint32_t q = 0; q < m;) {
        if (tot[q] > cap) {
            for (uint64_t lo = 0; lo < tot[q]; lo += cap) {
                p.blocks.push_back(IndexBlock{q, 1, (uint32_t)lo, (uint32_t)std::min<uint64_t>(cap, tot[q] - lo)});
                p.pieces++;
            }
            q++; p.query_blocks++;
            continue;
        }
        uint64_t sum = 0;
        uint32_t e = q;
        while (e < m && e - q < most && tot[e] <= cap && sum + tot[e] <= cap) sum += tot[e++];
        if (sum) p.blocks.push_back(IndexBlock{q, e - q, 0, (uint32_t)sum});
        q = e; p.query_blocks++;
    }
    for (const IndexBlock &b : p.blocks) { p.biggest = std::max(p.biggest, b.count); p.longest = std::max(p.longest, b.nq); }
    return p;
}

}  // namespace hulk
