// The host contraction of hulk_dendrogram (hulk_amd/csrc/hulk_boruvka.h) against a sequential Kruskal.  The offers a round of
// k_dendro_offer / k_dendro_fold delivers are produced here by a plain loop over a dense matrix: for sketch i the minimum of
// (w(i, p), p) over the p of another component whose w(i, p) = fmin(d(i, p), d(p, i)) is not NaN.  Rounds until one component is
// left or a round has no offer; the sorted edges must be Kruskal's on the pairs sorted by (w, lo, hi), the number of rounds at
// most ceil(log2 n) + 1, comp[] the smallest member of every component.  Then the refusals: an offer from outside the set, an offer
// from inside the sketch's own component.
// Stand-alone (tests/test_dendrogram_cpu.py builds it with -fsanitize=address,undefined and runs it); exit status 0 = all cases agree.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "hulk_boruvka.h"

using hulk::Boruvka;
using hulk::BoruvkaEdge;
using hulk::BORUVKA_NONE;

typedef std::vector<std::vector<double>> Matrix;                    // d[i][j], i the subject; NaN: no distance

static uint64_t bits(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }

static std::vector<BoruvkaEdge> kruskal(const Matrix &d) {
    const uint32_t n = (uint32_t)d.size();
    std::vector<BoruvkaEdge> all, out;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = i + 1; j < n; j++) {
            const double w = std::fmin(d[i][j], d[j][i]);
            if (w == w) all.push_back({bits(w), i, j});
        }
    std::sort(all.begin(), all.end());
    std::vector<uint32_t> p(n);
    std::iota(p.begin(), p.end(), 0u);
    auto find = [&](uint32_t x) { while (p[x] != x) x = p[x]; return x; };
    for (const BoruvkaEdge &e : all) {
        const uint32_t a = find(e.lo), b = find(e.hi);
        if (a != b) { p[std::max(a, b)] = std::min(a, b); out.push_back(e); }
    }
    return out;
}

static void offers(const Matrix &d, const std::vector<uint32_t> &comp, std::vector<uint64_t> &best_d, std::vector<uint32_t> &best_p) {
    const uint32_t n = (uint32_t)d.size();
    best_d.assign(n, BORUVKA_NONE); best_p.assign(n, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t p = 0; p < n; p++) {
            if (p == i || comp[p] == comp[i]) continue;
            const double w = std::fmin(d[i][p], d[p][i]);
            if (w != w) continue;
            if (bits(w) < best_d[i]) { best_d[i] = bits(w); best_p[i] = p; }       // (p ascends: the smaller partner at equal w)
        }
}

static bool run_case(const char *name, const Matrix &d) {
    const uint32_t n = (uint32_t)d.size();
    Boruvka f(n);
    std::vector<uint64_t> best_d; std::vector<uint32_t> best_p;
    uint32_t rounds = 0;
    bool ok = true;
    while (f.components > 1) {
        offers(d, f.comp, best_d, best_p);
        rounds++;
        const long added = f.contract(best_d.data(), best_p.data());
        if (added < 0) { ok = false; break; }
        if (added == 0) break;
    }
    f.finish();
    const std::vector<BoruvkaEdge> want = kruskal(d);
    uint32_t bound = 1;
    while ((1ull << (bound - 1)) < n) bound++;                      // ceil(log2 n) + 1
    ok = ok && f.edges == want && f.components == n - (uint32_t)want.size() && (n == 1 ? rounds == 0 : rounds <= bound);
    // comp: the smallest member of the component Kruskal's forest gives
    std::vector<uint32_t> p(n);
    std::iota(p.begin(), p.end(), 0u);
    auto find = [&](uint32_t x) { while (p[x] != x) x = p[x]; return x; };
    for (const BoruvkaEdge &e : want) { const uint32_t a = find(e.lo), b = find(e.hi); p[std::max(a, b)] = std::min(a, b); }
    for (uint32_t i = 0; i < n && ok; i++) ok = f.comp[i] == find(i);
    std::printf("%-34s n %5u edges %5zu (want %5zu) components %5u rounds %2u (bound %2u): %s\n", name, n, f.edges.size(), want.size(), f.components,
                rounds, bound, ok ? "ok" : "FAILED");
    return ok;
}

static bool run_refusal(const char *name, uint32_t partner_of_0, bool second_round) {
    Boruvka f(4);
    std::vector<uint64_t> bd(4, BORUVKA_NONE); std::vector<uint32_t> bp(4, 0xFFFFFFFFu);
    if (second_round) {                                             // 0 - 1 are one component, then 0 is offered 1 again
        bd[0] = bits(0.5); bp[0] = 1;
        if (f.contract(bd.data(), bp.data()) != 1) return false;
    }
    bd[0] = bits(0.25); bp[0] = partner_of_0;
    const bool ok = f.contract(bd.data(), bp.data()) == -1;
    std::printf("%-34s refused: %s\n", name, ok ? "ok" : "FAILED");
    return ok;
}

int main() {
    std::mt19937_64 rng(4711);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    bool ok = true;
    auto square = [](uint32_t n, double v) { return Matrix(n, std::vector<double>(n, v)); };
    for (uint32_t n : {1u, 2u, 3u, 64u, 257u}) {                    // heavy ties: distances are multiples of 1 / 8, symmetric
        Matrix d = square(n, 0.0);
        for (uint32_t i = 0; i < n; i++) for (uint32_t j = i + 1; j < n; j++) d[i][j] = d[j][i] = (double)(rng() % 9) / 8.0;
        ok &= run_case("ties, symmetric", d);
    }
    for (uint32_t n : {5u, 100u, 300u}) {                           // the two directions differ; a third of the entries NaN
        Matrix d = square(n, 0.0);
        for (uint32_t i = 0; i < n; i++) for (uint32_t j = 0; j < n; j++) d[i][j] = rng() % 3 == 0 ? nan : (double)(rng() % 1000) / 1000.0;
        ok &= run_case("asymmetric, NaN entries", d);
    }
    {   // NaN blocks: three groups with no distance between them, one sketch with none at all
        const uint32_t n = 200;
        Matrix d = square(n, nan);
        for (uint32_t i = 0; i + 1 < n; i++) for (uint32_t j = 0; j + 1 < n; j++) if (i % 3 == j % 3) d[i][j] = (double)(rng() % 5) / 4.0;
        ok &= run_case("NaN blocks and a loner", d);
    }
    ok &= run_case("every pair NaN", square(65, nan));
    ok &= run_case("all identical (star at 0)", square(65, 0.0));
    ok &= run_case("all disjoint (star at 0, w = 1)", square(65, 1.0));
    for (int order = 0; order < 3; order++) {                       // a path: neighbours at 1 / 4, everything else at 1
        const uint32_t n = 257;
        std::vector<uint32_t> at(n);
        std::iota(at.begin(), at.end(), 0u);
        if (order == 1) std::reverse(at.begin(), at.end());
        if (order == 2) std::shuffle(at.begin(), at.end(), rng);
        Matrix d = square(n, 1.0);
        for (uint32_t i = 0; i + 1 < n; i++) d[at[i]][at[i + 1]] = d[at[i + 1]][at[i]] = 0.25;
        ok &= run_case(order == 0 ? "path ascending" : order == 1 ? "path descending" : "path shuffled", d);
    }
    {   // a star on the LAST index at distinct heights, one direction only
        const uint32_t n = 129;
        Matrix d = square(n, nan);
        for (uint32_t i = 0; i + 1 < n; i++) d[n - 1][i] = (double)(n - i) / 256.0;
        ok &= run_case("star on the last index, one way", d);
    }
    ok &= run_refusal("partner outside the set", 4, false);
    ok &= run_refusal("partner in the own component", 1, true);
    return ok ? 0 : 1;
}
