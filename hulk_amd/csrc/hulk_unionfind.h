// hulk_unionfind.h — the lock-free union-find of k_cluster_link (hulk_cluster.hip).  HIP-free: the two atomics it needs are macros
// the including file defines, so tests/cpp/unionfind_host.cpp compiles this very text for the host and runs it on threads.
//   HULK_UF_LOAD(p)          relaxed atomic load of the uint32_t at p
//   HULK_UF_CAS(p, e, d)     atomic compare-and-swap on the uint32_t at p: stores d if it held e; returns the value it held
//   HULK_UF_FN               the function qualifiers (__device__ __forceinline__ / static inline)
// Invariant: parent[x] <= x, always; parent[x] == x makes x a root, and a root is hooked only UNDER A SMALLER INDEX, so the root of a
// component is its smallest member whatever the order of the unions.  A node that has stopped being a root never becomes one again,
// and every value parent[x] ever holds is an ancestor of x for ever: a stale read only makes a walk longer, and a hook on a node that
// is no longer a root fails its compare-and-swap.
// Every loop's variant is a strictly decreasing index: uf_find steps to a smaller index or stops, a failed hook continues from the
// smaller value the compare-and-swap returned.  A parent LARGER than its node cannot come from this code; it sets *err (to 1, by a
// compare-and-swap) and leaves every loop, so that corrupt memory ends the call and cannot spin it.
#ifndef HULK_UNIONFIND_H
#define HULK_UNIONFIND_H

#include <stdint.h>

// the root of x's component as of some moment during the call; path halving on the way (parent[x]: its parent -> its grandparent, an
// ancestor).  *bad: set when a parent larger than its node was read
HULK_UF_FN uint32_t uf_find(uint32_t *parent, uint32_t x, uint32_t *err, bool *bad) {
    for (;;) {
        const uint32_t p = HULK_UF_LOAD(&parent[x]);
        if (p == x) return x;
        if (p > x) { HULK_UF_CAS(err, 0u, 1u); *bad = true; return x; }
        const uint32_t g = HULK_UF_LOAD(&parent[p]);
        if (g == p) return p;
        if (g > p) { HULK_UF_CAS(err, 0u, 1u); *bad = true; return p; }
        HULK_UF_CAS(&parent[x], p, g);                               // (lost to another halving or not: both values are ancestors)
        x = g;                                                      // g < p < x
    }
}

// a and b are one component from here on
HULK_UF_FN void uf_unite(uint32_t *parent, uint32_t a, uint32_t b, uint32_t *err) {
    bool bad = false;
    for (;;) {
        a = uf_find(parent, a, err, &bad);
        b = uf_find(parent, b, err, &bad);
        if (bad || a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t was = HULK_UF_CAS(&parent[hi], hi, lo);
        if (was == hi) return;                                      // hooked: hi was a root
        if (was > hi) { HULK_UF_CAS(err, 0u, 1u); return; }
        a = was; b = lo;                                            // was < hi: somebody hooked hi first; a + b has decreased
    }
}

#endif
