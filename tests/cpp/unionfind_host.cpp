// The union-find of k_cluster_link (hulk_amd/csrc/hulk_unionfind.h) compiled for the host — the same text, the two atomics mapped to
// the compiler's builtins — and run by several threads at once over random and chain-shaped edge lists; the result must be the
// sequential union-find's: parent[x] <= x throughout, and after a flatten every label is the smallest member of its component.
// Then the error word: with a parent larger than its node planted, uf_find and uf_unite set it and return.
// Stand-alone (tests/test_cluster_cpu.py builds it with -fsanitize=address,undefined and runs it); exit status 0 = all cases agree.
//   unionfind_host [threads]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#define HULK_UF_FN static inline
#define HULK_UF_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)
static inline uint32_t host_cas(uint32_t *p, uint32_t e, uint32_t d) { __atomic_compare_exchange_n(p, &e, d, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED); return e; }
#define HULK_UF_CAS(p, e, d) host_cas((p), (e), (d))
#include "hulk_unionfind.h"

typedef std::vector<std::pair<uint32_t, uint32_t>> Edges;

static std::vector<uint32_t> sequential(uint32_t n, const Edges &edges) {
    std::vector<uint32_t> p(n);
    std::iota(p.begin(), p.end(), 0u);
    auto find = [&](uint32_t x) { while (p[x] != x) x = p[x]; return x; };
    for (const auto &e : edges) {
        const uint32_t a = find(e.first), b = find(e.second);
        if (a != b) p[std::max(a, b)] = std::min(a, b);
    }
    for (uint32_t i = 0; i < n; i++) p[i] = find(i);
    return p;
}

static bool run_case(const char *name, uint32_t n, const Edges &edges, unsigned threads) {
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    uint32_t err = 0;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; t++)
        th.emplace_back([&, t] { for (size_t i = t; i < edges.size(); i += threads) uf_unite(parent.data(), edges[i].first, edges[i].second, &err); });
    for (auto &x : th) x.join();
    bool ok = err == 0;
    for (uint32_t i = 0; i < n && ok; i++) ok = parent[i] <= i;
    std::vector<uint32_t> label(n);
    for (uint32_t i = 0; i < n && ok; i++) { bool bad = false; label[i] = uf_find(parent.data(), i, &err, &bad); ok = !bad; }
    const std::vector<uint32_t> want = sequential(n, edges);
    size_t differ = 0;
    for (uint32_t i = 0; i < n; i++) differ += label[i] != want[i];
    ok = ok && differ == 0;
    std::printf("%-28s n %7u edges %8zu threads %u: %s (%zu labels differ, err %u)\n", name, n, edges.size(), threads, ok ? "ok" : "FAILED", differ, err);
    return ok;
}

// the guard against corrupt memory: a parent LARGER than its node sets the error word and every loop is left — the call returns
static bool run_corrupt(const char *name, std::vector<uint32_t> parent, uint32_t a, uint32_t b, bool unite) {
    const std::vector<uint32_t> before = parent;
    uint32_t err = 0;
    bool bad = false;
    if (unite) uf_unite(parent.data(), a, b, &err);
    else (void)uf_find(parent.data(), a, &err, &bad);
    const bool ok = err == 1 && (unite || bad) && parent == before;     // (and nothing was hooked on the way out)
    std::printf("%-28s corrupt parent, %s(%u%s): %s (err %u)\n", name, unite ? "unite" : "find", a, unite ? (", " + std::to_string(b)).c_str() : "", ok ? "ok" : "FAILED", err);
    return ok;
}

int main(int argc, char **argv) {
    const unsigned threads = argc > 1 ? (unsigned)std::max(1, std::atoi(argv[1])) : 8;
    std::mt19937_64 rng(12345);
    bool ok = true;
    {   // sparse random graph: many components of a few members
        const uint32_t n = 20000; Edges e;
        for (uint32_t i = 0; i < n / 2; i++) e.emplace_back((uint32_t)(rng() % n), (uint32_t)(rng() % n));
        ok &= run_case("random sparse", n, e, threads);
    }
    {   // dense random graph: one giant component, the same roots contended by every thread
        const uint32_t n = 5000; Edges e;
        for (uint32_t i = 0; i < 20 * n; i++) e.emplace_back((uint32_t)(rng() % n), (uint32_t)(rng() % n));
        ok &= run_case("random dense", n, e, threads);
    }
    for (int order = 0; order < 3; order++) {   // a chain i - i+1: ascending, descending and shuffled (deep paths, halving)
        const uint32_t n = 30000; Edges e;
        for (uint32_t i = 0; i + 1 < n; i++) e.emplace_back(i, i + 1);
        if (order == 1) std::reverse(e.begin(), e.end());
        if (order == 2) std::shuffle(e.begin(), e.end(), rng);
        ok &= run_case(order == 0 ? "chain ascending" : order == 1 ? "chain descending" : "chain shuffled", n, e, threads);
    }
    {   // chains broken into pieces, every edge given twice and in both directions, self-loops between them
        const uint32_t n = 10000; Edges e;
        for (uint32_t i = 0; i + 1 < n; i++) if (i % 97 != 96) { e.emplace_back(i + 1, i); e.emplace_back(i, i + 1); }
        for (uint32_t i = 0; i < n; i += 5) e.emplace_back(i, i);
        std::shuffle(e.begin(), e.end(), rng);
        ok &= run_case("broken chains, duplicates", n, e, threads);
    }
    {   // a star on the LARGEST index: every hook moves the root down
        const uint32_t n = 8000; Edges e;
        for (uint32_t i = 0; i + 1 < n; i++) e.emplace_back(n - 1, i);
        std::shuffle(e.begin(), e.end(), rng);
        ok &= run_case("star on the last index", n, e, threads);
    }
    {   // one node
        ok &= run_case("one node", 1, Edges{{0u, 0u}}, threads);
    }
    {   // parent[5] = 9 > 5: met as a node's own parent, as a grandparent (7 -> 4 -> 8), and inside a union from either side
        const std::vector<uint32_t> own = {0, 1, 2, 3, 4, 9, 6, 7, 8, 9}, grand = {0, 1, 2, 3, 8, 5, 6, 4, 8, 9};
        ok &= run_corrupt("own parent", own, 5, 0, false);
        ok &= run_corrupt("grandparent", grand, 7, 0, false);
        ok &= run_corrupt("in a union", own, 2, 5, true) && run_corrupt("in a union", grand, 7, 1, true);
    }
    return ok ? 0 : 1;
}
