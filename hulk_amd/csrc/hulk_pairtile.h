// hulk_pairtile.h — the register tile of the pairwise distance kernels: HULKdata.GetDistance (sketchio.go:259-306) of 32 subject
// sketches against 64 other sketches, summed over the S slots in ascending order.  One text for
//   k_search_dist   (hulk_search.hip)    a block of queries against a strip of the database, either side the subject
//   k_cluster_link  (hulk_cluster.hip)   one set against itself in bands of subject rows; the distances go no further than a compare
//   k_links_count, k_links_fill (hulk_links.hip) the same bands; the distances go into a mask, then into the edges
//   k_dendro_offer  (hulk_dendrogram.hip) the same bands; the distances go into per-sketch minima
// each of which is a kernel template over the set type (PairSet below; BottomkSet, hulk_bottomk_tile.h, the bottom-k metric's):
// its index arithmetic, one call of SET::tile and its own epilogue over pair_distance<SET::METRIC>.
// k_smash (hulk_pairwise.hip: one set against itself, the whole N x N matrix) KEEPS A LOOP OF ITS OWN, the same text with `if`
// for `if constexpr`: through pair_tile its weighted form ran 1.1 % slower on the MI355X than with its own loop (N = 8,192,
// S = 512: 5.29e12 against 5.35e12 pair-slots/s, medians of six runs of nine each, the runs of either build within 0.7 % of
// each other; 1.0 % at S = 50; jaccard the same).  k_search_dist and k_cluster_link run weighted jaccard 1 - 2 % faster through
// it than with loops of their own and jaccard within 0.4 % either way, which is what k_smash, the same instructions in
// both libraries, shows between them too: profiles/pairtile.txt.  The slot loop is the same instructions in every one of
// these builds; what moves is the register allocation around it.  A change to the tile is made here AND in k_smash, and
// tests/test_gpu_pairtile.py holds the three kernels to one another bit for bit.  k_smash uses the constants and
// pair_distance of this header.
//
// Layout.  Both sides are SLOT-major doubles as k_smash_prep writes them: (double)min and |w| at [slot][sketch], the pitch a
// multiple of PAIR_TQ = 64 sketches, zeros in the rows behind the last sketch.  A workgroup of 128 threads owns a tile of
// PAIR_TS = 32 subjects x PAIR_TQ = 64 others, thread t the subjects 4 * (t / 16) + i and the others 4 * (t % 16) + j, i, j < 4.
// Chunks of PAIR_CH = 32 slots go through LDS as [slot][row] (the prepared layout: 16-byte loads in, 16-byte LDS stores, no
// transposition; rows padded by PAIR_PAD doubles) in two buffers: thread t moves slot t / 4 of a chunk — 8 subject rows (mins,
// weights) and 16 other rows from t % 4 on — and chunk n + 1 is loaded into registers before chunk n is computed and stored behind
// it, one barrier per chunk.  Per slot a thread reads its 4 subject mins, 4 subject weights and 4 other mins with six
// ds_read_b128 (0.375 LDS reads per (pair, slot)) and runs 16 independent accumulators; the slot loop is unrolled by two, so that
// the next slot's six LDS reads are in flight under this one's 72 VALU.
//
// Contract.
//   - The SUBJECT side brings mins, |w| and the union, the other side mins only: acc[i][j] += equal ? |w_subject| : 0.0 is the
//     reference's conditional add bit for bit (the sums are non-negative: x + 0.0 == x), and uni[i] is the sum of the subject's
//     |w| whatever the other sketch (both branches of distances.go:58-68 add max(wA, wB) = |w| when hsB is the subject,
//     sketchio.go:293-301).  METRIC 0 (jaccard) reads no weights (awT is not dereferenced) and counts the equal slots in cnt — a
//     count of 1.0s is exact in fp64; METRIC 1 (weighted jaccard) fills acc and uni.  The outputs of the other metric stay zero.
//   - The sums are taken in ASCENDING slot order, one accumulator a pair: the fp64 results are the Go loops', and every user's
//     distance for a pair is the same bits.
//   - Rows behind the last sketch and slots behind S contribute zeros: the former are zeros in the prepared arrays (a pair of
//     two such rows "agrees" in every slot — the caller stores or counts no pair outside its set), the latter are not loaded.
//   - What is read: of every slot's row the 32 subject columns from a_first and the 64 other columns from b_first on, and
//     nothing else.  a_first must be a multiple of 2 and b_first too (16-byte loads); both ranges must lie inside the
//     allocation.  With pitches and first columns that are multiples of 64 they lie inside the row.  hulk_search's query
//     blocks of 32 put a 64-wide tile of other columns in the middle of the last 64 columns of the queries' rows: it reads up
//     to 32 doubles past a slot's row — the next slot's, and behind the last slot the + 64 doubles of padding that caller owes.
//   - Every thread of the workgroup calls it, once (it holds barriers).  The last barrier stands behind the last read of the LDS
//     buffers: when the call returns, LDS is free for the caller's epilogue, and a __shared__ word the caller wrote before
//     the call is visible to the whole workgroup (k_cluster_link's wg_links relies on both).
//
// Resources (gfx950, hipcc -O3; DESIGN 4d has the table and the measurements): 116 - 121 VGPRs and 51,200 bytes of LDS for
// jaccard, two workgroups a SIMD; 200 - 204 VGPRs and 68,608 bytes for weighted jaccard, one; no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hulk {

constexpr int PAIR_TS = 32, PAIR_TQ = 64, PAIR_CH = 32, PAIR_PAD = 2;

// aT / awT: the subject side [S][AP], a_first its first column of this tile (the caller's origin + tile offset); bT: the other
// side [S][BP], b_first likewise.  Sets acc / uni (METRIC 1) or cnt (METRIC 0) of this thread's 4 x 4 pairs.
template <int METRIC>
__device__ __forceinline__ void pair_tile(const double *__restrict__ aT, const double *__restrict__ awT, uint32_t AP, uint32_t a_first,
                                          const double *__restrict__ bT, uint32_t BP, uint32_t b_first, uint32_t S,
                                          double (&acc)[4][4], double (&uni)[4], uint32_t (&cnt)[4][4]) {
    __shared__ __align__(16) double ma[2][PAIR_CH][PAIR_TS + PAIR_PAD], wa[METRIC == 1 ? 2 : 1][METRIC == 1 ? PAIR_CH : 1][PAIR_TS + PAIR_PAD];
    __shared__ __align__(16) double mb[2][PAIR_CH][PAIR_TQ + PAIR_PAD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;     // other quad, subject quad inside the tile
    // staging: thread t moves slot (t / 4) of the chunk: 8 subject rows (mins, weights) and 16 other rows from (t % 4) on
    const int lc = tid >> 2, lr = tid & 3;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uni[i] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) { acc[i][j] = 0.0; cnt[i][j] = 0; }
    }
    double2 ra[4], rw[4], rb[8];
    auto fetch = [&](uint32_t c0) {
        const uint32_t col = c0 + (uint32_t)lc;
        const bool ok = col < S;
        const double2 *pa = (const double2 *)(aT + (size_t)col * AP + a_first + 8 * lr);
        const double2 *pw = (const double2 *)(awT + (size_t)col * AP + a_first + 8 * lr);
        const double2 *pb = (const double2 *)(bT + (size_t)col * BP + b_first + 16 * lr);
#pragma unroll
        for (int x = 0; x < 4; x++) { ra[x] = ok ? pa[x] : make_double2(0.0, 0.0); if constexpr (METRIC == 1) rw[x] = ok ? pw[x] : make_double2(0.0, 0.0); }
#pragma unroll
        for (int x = 0; x < 8; x++) rb[x] = ok ? pb[x] : make_double2(0.0, 0.0);
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int x = 0; x < 4; x++) { *(double2 *)&ma[buf][lc][8 * lr + 2 * x] = ra[x]; if constexpr (METRIC == 1) *(double2 *)&wa[buf][lc][8 * lr + 2 * x] = rw[x]; }
#pragma unroll
        for (int x = 0; x < 8; x++) *(double2 *)&mb[buf][lc][16 * lr + 2 * x] = rb[x];
    };
    fetch(0);
    stash(0);
    __syncthreads();
    int buf = 0;
    for (uint32_t c0 = 0; c0 < S; c0 += PAIR_CH, buf ^= 1) {
        const bool more = c0 + PAIR_CH < S;
        if (more) fetch(c0 + PAIR_CH);                              // in flight under this chunk's arithmetic
        const uint32_t lim = S - c0 < (uint32_t)PAIR_CH ? S - c0 : (uint32_t)PAIR_CH;
#pragma unroll 2
        for (uint32_t c = 0; c < lim; c++) {
            const double2 a01 = *(const double2 *)&ma[buf][c][4 * ty], a23 = *(const double2 *)&ma[buf][c][4 * ty + 2];
            const double2 b01 = *(const double2 *)&mb[buf][c][4 * tx], b23 = *(const double2 *)&mb[buf][c][4 * tx + 2];
            const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
            if constexpr (METRIC == 1) {
                const double2 w01 = *(const double2 *)&wa[buf][c][4 * ty], w23 = *(const double2 *)&wa[buf][c][4 * ty + 2];
                const double w[4] = {w01.x, w01.y, w23.x, w23.y};
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    uni[i] += w[i];                                 // the subject's |w|, whatever the other sketch
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][j] += (a[i] == b[j]) ? w[i] : 0.0;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) cnt[i][j] += (a[i] == b[j]) ? 1u : 0u;      // a count of 1.0s is exact in fp64
            }
        }
        if (more) stash(buf ^ 1);                                   // (the other buffer: nobody reads it during this chunk)
        __syncthreads();
    }
}

// a prepared set [S][pitch] as the kernels see it (view(): from its two buffers, on the host or inside a kernel).  tile(): this set the subject side, `other` the other side (BottomkSet,
// hulk_bottomk_tile.h, has the same two members); SET::METRIC is the pair_distance of the epilogue
template <int M>
struct PairSet {
    static constexpr int METRIC = M;
    const double *mT, *wT;
    uint32_t pitch;
    static __host__ __device__ PairSet view(const double *d_mT, const double *d_wT, uint32_t rows, uint32_t) { return PairSet{d_mT, d_wT, rows}; }
    __device__ __forceinline__ void tile(uint32_t a_first, const PairSet &other, uint32_t b_first, uint32_t S, double (&acc)[4][4],
                                         double (&uni)[4], uint32_t (&cnt)[4][4]) const {
        pair_tile<M>(mT, wT, pitch, a_first, other.mT, other.pitch, b_first, S, acc, uni, cnt);
    }
};

// the distance of one pair from the tile's sums: the expression every user stores or compares, so that a pair's distance is the
// same bits in hulk_smash's matrix, in a search's list and against a clustering's threshold.  (Where the weighted quotient is
// 0 / 0 or Inf / Inf the NaN is the GPU division's, without the sign bit of the amd64 one: k_snap_panel sets it, these do not)
template <int METRIC>
__device__ __forceinline__ double pair_distance(double acc, double uni, uint32_t cnt, uint32_t S) {
    return METRIC == 1 ? 1 - (acc / uni) : 1.0 - ((double)cnt / (double)S);
}

}  // namespace hulk
