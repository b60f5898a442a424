// hulk_bottomk_merge.h — the arithmetic of the bottom-k metric (HULK_METRIC_BOTTOMK): KMVsketch.GetSimilarity (kmv.go:119-159), the
// multiset intersection of two lists of uint64.  HIP-free: HULK_BK_FN holds the function qualifiers (__device__ __forceinline__ /
// static inline), so tests/cpp/bottomk_host.cpp compiles this very text for the host, under the sanitizers.
// A sketch is prepared ONCE into run-length form: its DISTINCT values strictly ascending, val[0 .. len), and how often each occurs,
// mult[0 .. len) (the multiplicities add up to the sketch size).  In that form
//   intersect(A, B) = the sum over the values both lists hold of min(mult_A, mult_B)
// which is what the map-and-decrement loop of kmv.go:143-156 counts, is one two-pointer merge (bottomk_merge), and is ADDITIVE over
// disjoint ranges of values: the tile (hulk_bottomk_tile.h) cuts all its lists at shared pivots and merges window by window.
// Strictly ascending values are what makes the cut exact — "the entries <= pivot" (bottomk_upto) never splits a run — and
// what makes it progress: the list whose last window entry is the pivot consumes its whole window.
#ifndef HULK_BOTTOMK_MERGE_H
#define HULK_BOTTOMK_MERGE_H

#include <stdint.h>

// sum of min(am, bm) over the values common to av[0 .. na) and bv[0 .. nb), both strictly ascending
HULK_BK_FN uint32_t bottomk_merge(const uint64_t *av, const uint32_t *am, uint32_t na, const uint64_t *bv, const uint32_t *bm, uint32_t nb) {
    uint32_t ia = 0, ib = 0, cnt = 0;
    while (ia < na && ib < nb) {
        const uint64_t a = av[ia], b = bv[ib];
        if (a == b) cnt += am[ia] < bm[ib] ? am[ia] : bm[ib];
        ia += a <= b;
        ib += b <= a;
    }
    return cnt;
}

// how many of the strictly ascending v[0 .. n) are <= pivot
HULK_BK_FN uint32_t bottomk_upto(const uint64_t *v, uint32_t n, uint64_t pivot) {
    uint32_t lo = 0, hi = n;                                        // v[0 .. lo) <= pivot < v[hi .. n)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (v[mid] <= pivot) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The sorting network of k_bottomk_prep over n values, n any number: stages of block size k = 2, 4, .. (the first power of two that
// is not below n); a stage is one FLIP step (j == 0: position x of a block against position k - 1 - x) and the DISPERSE steps j = k / 4,
// k / 8, .. 1 (x against x + j inside blocks of 2 * j).  Comparator t < p2 / 2 of a step takes positions *lo < *hi, the smaller value
// to *lo.  Every comparator points the same way, so values that stood behind n — "plus infinity" — would never move: a comparator
// whose *hi is not below n is SKIPPED, and the network sorts n values exactly as it sorts p2 with that padding.
HULK_BK_FN void bottomk_net_pair(uint32_t t, uint32_t k, uint32_t j, uint32_t *lo, uint32_t *hi) {
    if (j == 0) {
        const uint32_t h = k >> 1, base = (t / h) * k, x = t % h;
        *lo = base + x; *hi = base + k - 1 - x;
    } else {
        *lo = (t / j) * 2 * j + t % j; *hi = *lo + j;
    }
}

#endif
