// hulk_bottomk.hip — the bottom-k metric (HULK_METRIC_BOTTOMK): KMVsketch.GetSimilarity (kmv.go:119-159), the multiset intersection
// of two KMV value lists over their length, as a distance.  Lists of EQUAL length only, as everywhere in this library (the loader's
// "sketch length mismatch" rule, the rectangular [n][S] arrays); the unequal lengths GetSimilarity tolerates are out of scope.
//   k_bottomk_prep    once per set or per search strip, one workgroup a sketch: sorts the S <= 4096 values ascending in LDS — the
//                     caller's order does not matter — and writes the run-length form the tile reads (hulk_bottomk_tile.h: distinct
//                     values, multiplicities, their number).  The network is bottomk_net_pair's (hulk_bottomk_merge.h): any S, no
//                     padding values, so the largest uint64 is a value like any other
//   k_bottomk_matrix  the N x N matrix of hulk_smash: bottomk_tile over one set and pair_distance<0>; every pair with both sketches
//                     below N is stored (the full square: the tile is symmetric, the matrix is written whole)
//   k_bottomk_global  the obvious fallback, kept as the yardstick of tools/profile_bottomk.py: a thread a pair, bottomk_merge over the
//                     prepared lists where they lie in global memory.  The profiling build runs it with HULK_BOTTOMK_GLOBAL
// k_search_dist, k_cluster_link, k_links_count, k_links_fill and k_dendro_offer run the tile as their BottomkSet instances, in their units.
#include "../../include/hulk_hip.h"
#include "hulk_device.h"
#include "hulk_bottomk_tile.h"

#include <stdlib.h>

namespace hulk {
namespace {

constexpr uint32_t BK_MAX_S = HULK_MINHASH_MAX_SKETCH, BK_PREP_THREADS = 256;

// mins [N][S] as the caller gave them -> val / mult [rows][S], len [rows]; gridDim.x = rows, a row behind N gets len 0
__global__ __launch_bounds__(256) void k_bottomk_prep(const unsigned long long *__restrict__ mins, uint32_t N, uint32_t S,
                                                      uint64_t *__restrict__ val, uint32_t *__restrict__ mult, uint32_t *__restrict__ len) {
    __shared__ uint64_t sv[BK_MAX_S];
    __shared__ uint32_t pos[BK_MAX_S + 1];                          // where run d starts; pos[runs] = S
    __shared__ uint32_t heads[BK_PREP_THREADS], runs;
    const uint32_t row = blockIdx.x, tid = threadIdx.x;
    if (row >= N) { if (tid == 0) len[row] = 0; return; }           // (the whole workgroup)
    for (uint32_t c = tid; c < S; c += BK_PREP_THREADS) sv[c] = mins[(size_t)row * S + c];
    __syncthreads();
    uint32_t p2 = 1;
    while (p2 < S) p2 <<= 1;
    for (uint32_t k = 2; k <= p2; k <<= 1)
        for (uint32_t j = 0;;) {                                    // the flip step, then k / 4, k / 8, .. 1
            for (uint32_t t = tid; t < p2 / 2; t += BK_PREP_THREADS) {
                uint32_t lo, hi;
                bottomk_net_pair(t, k, j, &lo, &hi);
                if (hi < S) {
                    const uint64_t a = sv[lo], b = sv[hi];
                    if (b < a) { sv[lo] = b; sv[hi] = a; }
                }
            }
            __syncthreads();
            j = j ? j >> 1 : k >> 2;
            if (!j) break;
        }
    // run heads: a thread takes E consecutive positions, its runs start behind those of the threads in front of it
    const uint32_t E = (S + BK_PREP_THREADS - 1) / BK_PREP_THREADS, i0 = tid * E, i1 = i0 + E < S ? i0 + E : S;
    uint32_t h = 0;
    for (uint32_t i = i0; i < i1; i++) h += (i == 0 || sv[i] != sv[i - 1]) ? 1u : 0u;
    heads[tid] = h;
    __syncthreads();
    uint32_t d = 0;
    for (uint32_t x = 0; x < tid; x++) d += heads[x];
    for (uint32_t i = i0; i < i1; i++)
        if (i == 0 || sv[i] != sv[i - 1]) { val[(size_t)row * S + d] = sv[i]; pos[d] = i; d++; }
    if (tid == BK_PREP_THREADS - 1) { pos[d] = S; runs = d; len[row] = d; }
    __syncthreads();
    for (uint32_t x = tid; x < runs; x += BK_PREP_THREADS) mult[(size_t)row * S + x] = pos[x + 1] - pos[x];
}

__global__ __launch_bounds__(128) void k_bottomk_matrix(const BottomkSet set, uint32_t N, uint32_t S, double *__restrict__ out) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint32_t s0 = blockIdx.y * PAIR_TS, q0 = blockIdx.x * PAIR_TQ;
    uint32_t cnt[4][4];
    bottomk_tile(set, s0, set, q0, S, cnt);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t s = s0 + 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t q = q0 + 4 * tx + j;
            if (s < N && q < N) out[(size_t)s * N + q] = pair_distance<0>(0.0, 0.0, cnt[i][j], S);
        }
    }
}

__global__ __launch_bounds__(256) void k_bottomk_global(const BottomkSet set, uint32_t N, uint32_t S, double *__restrict__ out) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (q >= N) return;
    const uint32_t cnt = bottomk_merge(set.val + (size_t)s * S, set.mult + (size_t)s * S, set.len[s],
                                       set.val + (size_t)q * S, set.mult + (size_t)q * S, set.len[q]);
    out[(size_t)s * N + q] = pair_distance<0>(0.0, 0.0, cnt, S);
}

}  // namespace

// N sketches of d_mins [N][S] -> the prepared form in d_mT / d_wT (BottomkSet::view over smash_padded_n(N) rows).  S <= 4096: the caller checks
hipError_t launch_bottomk_prep(hipStream_t s, const unsigned long long *d_mins, uint32_t N, uint32_t S, double *d_mT, double *d_wT) {
    if (N == 0 || S == 0 || S > BK_MAX_S) return N == 0 || S == 0 ? hipSuccess : hipErrorInvalidValue;
    const uint32_t rows = smash_padded_n(N);
    hipLaunchKernelGGL(k_bottomk_prep, dim3(rows), dim3(BK_PREP_THREADS), 0, s, d_mins, N, S, bottomk_val(d_mT), bottomk_mult(d_wT),
                       bottomk_len(d_wT, rows, S));
    return hipGetLastError();
}

// the matrix of hulk_smash for HULK_METRIC_BOTTOMK: d_mins [N][S] -> d_out [N][N]; d_mT, d_wT: scratch of smash_padded_n(N) * S doubles each
hipError_t launch_bottomk_smash(hipStream_t s, const unsigned long long *d_mins, uint32_t N, uint32_t S, double *d_out, double *d_mT,
                                double *d_wT) {
    if (N == 0 || S == 0) return hipSuccess;
    const uint32_t rows = smash_padded_n(N);
    hipError_t e = launch_bottomk_prep(s, d_mins, N, S, d_mT, d_wT);
    if (e != hipSuccess) return e;
    const BottomkSet set = BottomkSet::view(d_mT, d_wT, rows, S);
    // experiment (tools/profile_bottomk.py, the profiling build only): 1 = the merge from global memory, 2 = the preparation alone
    const char *exp = HULK_EXP_ENV("HULK_BOTTOMK_GLOBAL");
    const int mode = exp ? atoi(exp) : 0;
    if (mode == 2) return hipSuccess;
    if (mode == 1 && N > 65535) return hipErrorInvalidValue;       // (grid.y)
    if (mode == 1) hipLaunchKernelGGL(k_bottomk_global, dim3((N + 255) / 256, N), dim3(256), 0, s, set, N, S, d_out);
    else hipLaunchKernelGGL(k_bottomk_matrix, dim3(rows / PAIR_TQ, (N + PAIR_TS - 1) / PAIR_TS), dim3(128), 0, s, set, N, S, d_out);
    return hipGetLastError();
}

}  // namespace hulk
