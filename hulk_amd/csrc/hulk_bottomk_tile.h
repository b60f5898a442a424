// hulk_bottomk_tile.h — the tile of the bottom-k metric (HULK_METRIC_BOTTOMK, include/hulk_hip.h): the multiset intersection of
// KMVsketch.GetSimilarity (kmv.go:119-159) for 32 subject sketches against 64 other sketches.  It hands the calling thread cnt[4][4]
// in pair_tile's thread-to-pair mapping (hulk_pairtile.h: 128 threads, thread t the subjects 4 * (t / 16) + i and the others
// 4 * (t % 16) + j), so k_search_dist, k_cluster_link, k_links_count, k_links_fill and k_dendro_offer run it as BottomkSet::tile
// under their one epilogue, with pair_distance<0>: the distance is 1.0 - (double)cnt / (double)S, jaccard's expression over another
// count.
//
// Layout (k_bottomk_prep, hulk_bottomk.hip, once per set or strip).  SKETCH-major, run-length form (hulk_bottomk_merge.h): val[row][S]
// the row's distinct values strictly ascending, mult[row][S] their multiplicities, len[row] how many there are (<= S; what lies
// behind is never read).  Values are uint64 and are compared as such: 2^60 and 2^60 + 1 differ.  The arrays hold the padded
// number of rows (smash_padded_n, a multiple of 64); a row behind the last sketch has len 0 and intersects nothing.  The three
// arrays live in the two buffers of 8 * S * rows bytes the other metrics keep their slot-major doubles in: BottomkSet::view.
//
// The tile.  96 lists of S = 512 values are 393 KB, the LDS holds 160 KiB: the lists go through it in WINDOWS between shared pivots,
// which the count allows because it is additive over disjoint ranges of values.  Every list has a cursor, 0 at the start.  A round
//   1. loads the next BK_W = 32 entries of every list from its cursor on (fewer where the list ends) — thread t entry t % 32 of
//      lists t / 32, t / 32 + 4, ..: 256 contiguous bytes a list;
//   2. takes the pivot: the smallest of the LAST window entries of the lists that go on behind their window (thread l < 96 reads
//      list l's, a wave minimum, two words through LDS).  No such list: the pivot is the largest uint64 and this is the last round;
//   3. counts per list the window entries <= pivot (thread l < 96, a binary search) and moves the cursor behind them.  Values
//      ascend strictly, so every entry <= pivot of every list is inside its window: the entries behind a window are larger than its last
//      one, which is not below the pivot;
//   4. merges, per thread, its 16 pairs over those prefixes: 16 two-pointer merges advanced side by side, one step of each per
//      iteration (16 independent chains of two LDS reads and a compare), until the slowest has ended.
// Three barriers a round; the last stands behind the last LDS read, so LDS is free for the caller's epilogue when the call returns
// and a __shared__ word the caller wrote before the call is visible to the workgroup, as with pair_tile.
// Progress: the list that supplied the pivot consumes its whole window.  With lists of like density (hash values) a round
// advances the lists by about half a window (the pivot is the smallest of 96 order statistics), S / 16 rounds or so; lists of very
// different density take more, shorter rounds — at most one per window of any list, 96 * S / 32 — and stay exact.  Any 0 <= len <= S
// goes the same way, S = 1 .. HULK_MINHASH_MAX_SKETCH.  No atomics.
//
// What is read: rows a_first .. a_first + 31 of A and b_first .. b_first + 63 of B (len, and val / mult below len); both ranges
// must lie inside the padded arrays.  Every thread of the workgroup calls it, once.
//
// Resources (gfx950, hipcc -O3; DESIGN 4g has the table and the measurements): 39,192 bytes of LDS, four workgroups a CU; 128 VGPRs
// under the matrix, search and cluster epilogues, 130 under the dendrogram's; no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hulk_pairtile.h"

#define HULK_BK_FN __device__ __forceinline__
#include "hulk_bottomk_merge.h"

namespace hulk {

constexpr int BK_W = 32, BK_PITCH = BK_W + 1, BK_LISTS = PAIR_TS + PAIR_TQ;

// a prepared set as the kernels take it, PairSet's counterpart (hulk_pairtile.h): tile() is bottomk_tile below and leaves acc / uni
// as they are; METRIC 0, because pair_distance<0> is the distance and the count is symmetric as jaccard's is
struct BottomkSet {
    static constexpr int METRIC = 0;
    const uint64_t *val; const uint32_t *mult; const uint32_t *len;
    static __host__ __device__ BottomkSet view(const double *d_mT, const double *d_wT, uint32_t rows, uint32_t S);
    __device__ __forceinline__ void tile(uint32_t a_first, const BottomkSet &other, uint32_t b_first, uint32_t S, double (&)[4][4],
                                         double (&)[4], uint32_t (&cnt)[4][4]) const;
};

// the prepared form inside the two buffers of rows * S doubles each that the other metrics call mT and wT (rows = smash_padded_n(n)):
// val fills the first, mult the first half of the second, len stands behind mult (4 * rows bytes of the other half: S >= 1)
inline uint64_t *bottomk_val(double *d_mT) { return (uint64_t *)d_mT; }
inline uint32_t *bottomk_mult(double *d_wT) { return (uint32_t *)d_wT; }
inline uint32_t *bottomk_len(double *d_wT, uint32_t rows, uint32_t S) { return (uint32_t *)d_wT + (size_t)rows * S; }
inline __host__ __device__ BottomkSet BottomkSet::view(const double *d_mT, const double *d_wT, uint32_t rows, uint32_t S) {
    return BottomkSet{(const uint64_t *)d_mT, (const uint32_t *)d_wT, (const uint32_t *)d_wT + (size_t)rows * S};
}

// Sets cnt of this thread's 4 x 4 pairs: rows a_first + 4 * (t / 16) + i of A against rows b_first + 4 * (t % 16) + j of B
__device__ __forceinline__ void bottomk_tile(const BottomkSet A, uint32_t a_first, const BottomkSet B, uint32_t b_first, uint32_t S,
                                             uint32_t (&cnt)[4][4]) {
    __shared__ uint64_t wv[BK_LISTS][BK_PITCH];                     // (the pad column: a cursor that has reached BK_W reads it, unused)
    __shared__ uint32_t wm[BK_LISTS][BK_PITCH];
    __shared__ uint32_t s_cur[BK_LISTS], s_len[BK_LISTS], s_n[BK_LISTS];
    __shared__ uint64_t s_piv[2];
    __shared__ uint32_t s_more[2];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;     // other quad, subject quad inside the tile
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) cnt[i][j] = 0;
    // thread l < 96 keeps list l: subjects first, then the others
    const bool lister = tid < BK_LISTS;
    const BottomkSet &mine = tid < PAIR_TS ? A : B;
    const uint32_t my_row = tid < PAIR_TS ? a_first + (uint32_t)tid : b_first + (uint32_t)(tid - PAIR_TS);
    const uint32_t my_len = lister ? mine.len[my_row] : 0u;
    uint32_t my_cur = 0;
    if (lister) { s_cur[tid] = 0; s_len[tid] = my_len; }
    __syncthreads();
    for (;;) {
        for (int idx = tid; idx < BK_LISTS * BK_W; idx += 128) {
            const int l = idx / BK_W, e = idx % BK_W;
            const uint32_t pos = s_cur[l] + (uint32_t)e;
            if (pos < s_len[l]) {
                const BottomkSet &set = l < PAIR_TS ? A : B;
                const size_t at = (size_t)(l < PAIR_TS ? a_first + (uint32_t)l : b_first + (uint32_t)(l - PAIR_TS)) * S + pos;
                wv[l][e] = set.val[at];
                wm[l][e] = set.mult[at];
            }
        }
        uint64_t cand = ~0ull;
        const bool more = lister && my_cur + (uint32_t)BK_W < my_len;
        if (more) cand = mine.val[(size_t)my_row * S + my_cur + (uint32_t)BK_W - 1];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint64_t x = __shfl_xor(cand, o); cand = x < cand ? x : cand; }
        const uint32_t wave_more = __any(more) ? 1u : 0u;
        if ((tid & 63) == 0) { s_piv[tid >> 6] = cand; s_more[tid >> 6] = wave_more; }
        __syncthreads();                                            // the windows, the two minima
        const uint64_t pivot = s_piv[0] < s_piv[1] ? s_piv[0] : s_piv[1];
        const bool again = (s_more[0] | s_more[1]) != 0;            // (the whole workgroup reads the same two words)
        if (lister) {
            const uint32_t left = my_len - my_cur, n = left < (uint32_t)BK_W ? left : (uint32_t)BK_W;
            const uint32_t k = bottomk_upto(wv[tid], n, pivot);
            s_n[tid] = k;
            my_cur += k;
            s_cur[tid] = my_cur;                                    // (read again behind the round's last barrier)
        }
        __syncthreads();
        uint32_t na[4], nb[4], ia[16], ib[16];
#pragma unroll
        for (int i = 0; i < 4; i++) { na[i] = s_n[4 * ty + i]; nb[i] = s_n[PAIR_TS + 4 * tx + i]; }
#pragma unroll
        for (int p = 0; p < 16; p++) { ia[p] = 0; ib[p] = 0; }
        for (;;) {
            bool any = false;
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int p = 4 * i + j, ra = 4 * ty + i, rb = PAIR_TS + 4 * tx + j;
                    const bool act = ia[p] < na[i] && ib[p] < nb[j];
                    const uint64_t a = wv[ra][ia[p]], b = wv[rb][ib[p]];            // (behind a prefix: an entry nobody uses)
                    if (act) {
                        if (a == b) { const uint32_t x = wm[ra][ia[p]], y = wm[rb][ib[p]]; cnt[i][j] += x < y ? x : y; }
                        ia[p] += a <= b;
                        ib[p] += b <= a;
                        any = true;
                    }
                }
            if (!any) break;
        }
        __syncthreads();                                            // the windows and s_n are free
        if (!again) break;
    }
}

__device__ __forceinline__ void BottomkSet::tile(uint32_t a_first, const BottomkSet &other, uint32_t b_first, uint32_t S, double (&)[4][4],
                                                 double (&)[4], uint32_t (&cnt)[4][4]) const {
    bottomk_tile(*this, a_first, other, b_first, S, cnt);
}

}  // namespace hulk
