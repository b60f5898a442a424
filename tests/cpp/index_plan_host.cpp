// hulk_index_plan.h on the host (it is HIP-free): the block and launch plan of hulk_index_search at sizes no test can allocate on a
// device, under ASan / UBSan.  For every case: every launch the plan implies stays below 2^32 threads (a wave of 64 per (query, band)
// of a probe launch and per candidate of a verification launch); the blocks are in query order, a block of several queries holds
// exactly their candidates and no more than the cap; the pieces of a query tile [0, tot) in order; a query with candidates is in
// exactly one block or one run of pieces.  Prints "<case>: ok" per case.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "hulk_index_plan.h"

using namespace hulk;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s line %d: %s\n", name.c_str(), __LINE__, #cond); failures++; return; } } while (0)

static bool launch_ok(uint64_t waves) { return waves * 64 < (1ull << 32) && (waves + 3) / 4 < (1ull << 31); }

static void run(const std::string &name, const std::vector<uint32_t> &tot, uint32_t B, uint64_t scratch) {
    const uint32_t m = (uint32_t)tot.size(), cap = index_block_cap(scratch);
    CHECK(cap >= 1 && cap <= INDEX_MAX_WAVES && launch_ok(cap));
    // the count pass
    const uint32_t chunk = index_count_chunk(B);
    CHECK(chunk >= 1 && launch_ok((uint64_t)chunk * B));
    const IndexPlan p = index_plan(tot.data(), m, B, cap);
    uint32_t next = 0;                                              // the first query no block has covered yet
    uint64_t covered = 0, total = 0, pieces = 0;
    for (uint32_t q = 0; q < m; q++) total += tot[q];
    for (size_t i = 0; i < p.blocks.size(); i++) {
        const IndexBlock &b = p.blocks[i];
        CHECK(b.nq >= 1 && b.count >= 1 && b.count <= cap && (uint64_t)b.q0 + b.nq <= m);
        CHECK(launch_ok((uint64_t)b.nq * B) && launch_ok(b.count) && launch_ok(b.nq));
        CHECK(b.count <= p.biggest && b.nq <= p.longest);
        if (tot[b.q0] > cap) {                                      // a piece
            CHECK(b.nq == 1);
            const bool first = b.lo == 0;
            if (first) { for (uint32_t q = next; q < b.q0; q++) CHECK(tot[q] == 0); }
            else CHECK(i > 0 && p.blocks[i - 1].q0 == b.q0 && (uint64_t)p.blocks[i - 1].lo + p.blocks[i - 1].count == b.lo);
            CHECK((uint64_t)b.lo + b.count <= tot[b.q0]);
            const bool last = (uint64_t)b.lo + b.count == tot[b.q0];
            CHECK(last || b.count == cap);
            if (last) next = b.q0 + 1; else CHECK(i + 1 < p.blocks.size() && p.blocks[i + 1].q0 == b.q0);
            pieces++;
        } else {
            CHECK(b.lo == 0);
            for (uint32_t q = next; q < b.q0; q++) CHECK(tot[q] == 0);
            uint64_t sum = 0;
            for (uint32_t q = b.q0; q < b.q0 + b.nq; q++) { CHECK(tot[q] <= cap); sum += tot[q]; }
            CHECK(sum == b.count);
            next = b.q0 + b.nq;
        }
        covered += b.count;
    }
    for (uint32_t q = next; q < m; q++) CHECK(tot[q] == 0);
    CHECK(covered == total && pieces == p.pieces && p.query_blocks >= 1);
    std::printf("%s: ok (%zu blocks, %u pieces, longest %u, biggest %u)\n", name.c_str(), p.blocks.size(), p.pieces, p.longest, p.biggest);
}

int main() {
    uint64_t s = 88172645463325252ull;
    auto rnd = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    // the tests' shape: a handful of candidates, a scratch of 64
    { std::vector<uint32_t> t(1100); for (auto &x : t) x = (uint32_t)(rnd() % 4 == 0 ? rnd() % 500 : 0); run("small scratch", t, 15, 16 * 64); }
    // 2^20 queries x 103 bands: m B = 2^26.7, the count pass and the blocks' fill must be cut (index_count_chunk(103) = 325 771 queries)
    { std::vector<uint32_t> t(1u << 20); for (auto &x : t) x = (uint32_t)(rnd() % 40); run("2^20 queries, 103 bands, sparse", t, 103, 0 + (256ull << 20)); }
    // nothing is a candidate anywhere: no block at all
    { std::vector<uint32_t> t(1u << 20, 0); run("no candidates", t, 103, 256ull << 20); }
    // a dense collection under a scratch of 16 GiB: the cap is the launch limit, not the scratch
    { std::vector<uint32_t> t(4096); for (auto &x : t) x = 60000 + (uint32_t)(rnd() % 5000); run("dense, 16 GiB of scratch", t, 103, 16ull << 30); }
    // queries above the cap between queries below it, and a query of 2^32 - 2 candidates
    { std::vector<uint32_t> t(2000); for (size_t i = 0; i < t.size(); i++) t[i] = i % 7 == 3 ? (1u << 26) + (uint32_t)(rnd() % 1000) : (uint32_t)(rnd() % 100000);
      t[1000] = 0xFFFFFFFEu; run("pieces at the launch limit", t, 52, 1ull << 40); }
    // the most bands: chunks of 512 queries
    { std::vector<uint32_t> t(65536); for (auto &x : t) x = (uint32_t)(rnd() % 3); run("65535 bands", t, 65535, 256ull << 20); }
    // one candidate of room
    { std::vector<uint32_t> t(300); for (auto &x : t) x = (uint32_t)(rnd() % 5); run("a scratch of one candidate", t, 4, 16); }
    if (!(index_threads_ok(41698000ull, 103) && !index_threads_ok(41698000ull, 104) && !index_threads_ok(1ull << 32, 1) && index_threads_ok((1ull << 32) - 1, 1))) {
        std::printf("FAILED index_threads_ok\n"); failures++;
    } else std::printf("index_threads_ok: ok\n");
    return failures ? 1 : 0;
}
