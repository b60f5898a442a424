// hulk_boruvka.h — the host side of hulk_dendrogram (hulk_dendrogram.hip): Boruvka's contraction of one round's offers.  HIP-free,
// plain C++: tests/cpp/boruvka_host.cpp compiles this very text and runs it against a sequential Kruskal.
// An OFFER to sketch i is its best edge out of its component: (d, partner), the lexicographic minimum over every sketch of ANOTHER
// component that has a distance to i — d as the bits of a non-negative, non-NaN double (they order like the value), partner the
// smaller index at equal d.  "No offer" is BORUVKA_NONE in the distance bits.
// Edges are totally ordered by the key (d, lo, hi), lo = min(i, partner), hi = max(i, partner).  For one sketch that key orders its
// partners like (d, partner), which is why a per-sketch minimum of (d, partner) loses nothing; for a COMPONENT the members differ,
// so its pick is the minimum of its members' offers by the EDGE key.  Under a total order the lightest edge out of a component is in
// the one minimum spanning forest (the cut property), so every pick is an edge of the result, the picks of one round close no cycle,
// and the forest does not depend on how many distances tie.  Two components may pick the same edge: it is one edge.
// Every component that has any edge out merges in every round that delivers offers, so their number at least halves: at most
// ceil(log2 n) such rounds; a round without any offer says that what is left is separated by NaNs.
#ifndef HULK_BORUVKA_H
#define HULK_BORUVKA_H

#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

namespace hulk {

constexpr uint64_t BORUVKA_NONE = ~0ull;

struct BoruvkaEdge {
    uint64_t d;                                                     // the distance's bits
    uint32_t lo, hi;
    bool operator<(const BoruvkaEdge &o) const { return d != o.d ? d < o.d : lo != o.lo ? lo < o.lo : hi < o.hi; }
    bool operator==(const BoruvkaEdge &o) const { return d == o.d && lo == o.lo && hi == o.hi; }
};

struct Boruvka {
    std::vector<uint32_t> comp;                                     // comp[i]: the smallest member of i's component
    std::vector<BoruvkaEdge> edges;                                 // the forest so far, in the order the rounds found it
    uint32_t components;

    explicit Boruvka(uint32_t n) : comp(n), components(n) { std::iota(comp.begin(), comp.end(), 0u); }

    // One round's offers (best_d / best_p, n entries each) -> the edges they add; comp is rewritten.  Returns the number of new
    // edges (0: no offer at all, the forest is complete), or -1 for an offer this code cannot have produced (a partner outside
    // the set or inside the sketch's own component): corrupt input ends the call and cannot spin it.
    long contract(const uint64_t *best_d, const uint32_t *best_p) {
        const uint32_t n = (uint32_t)comp.size();
        const BoruvkaEdge none = {BORUVKA_NONE, 0, 0};
        std::vector<BoruvkaEdge> pick(n, none);                     // indexed by the component's smallest member
        for (uint32_t i = 0; i < n; i++) {
            if (best_d[i] == BORUVKA_NONE) continue;
            const uint32_t p = best_p[i];
            if (p >= n || comp[p] == comp[i]) return -1;
            const BoruvkaEdge e = {best_d[i], std::min(i, p), std::max(i, p)};
            if (e < pick[comp[i]]) pick[comp[i]] = e;
        }
        std::vector<BoruvkaEdge> fresh;
        for (uint32_t c = 0; c < n; c++) if (pick[c].d != BORUVKA_NONE) fresh.push_back(pick[c]);
        std::sort(fresh.begin(), fresh.end());
        fresh.erase(std::unique(fresh.begin(), fresh.end()), fresh.end());
        // unite over the components' smallest members: the smaller one stays a root, so a root is its component's smallest member
        std::vector<uint32_t> up(n);
        std::iota(up.begin(), up.end(), 0u);
        auto find = [&](uint32_t x) { while (up[x] != x) { up[x] = up[up[x]]; x = up[x]; } return x; };
        for (const BoruvkaEdge &e : fresh) {
            const uint32_t a = find(comp[e.lo]), b = find(comp[e.hi]);
            if (a == b) return -1;                                  // (a cycle among the picks: the order was not total)
            up[std::max(a, b)] = std::min(a, b);
            edges.push_back(e);
        }
        for (uint32_t i = 0; i < n; i++) comp[i] = find(comp[i]);
        components -= (uint32_t)fresh.size();
        return (long)fresh.size();
    }

    // the merge order of the dendrogram: ascending by the key
    void finish() { std::sort(edges.begin(), edges.end()); }
};

}  // namespace hulk

#endif
