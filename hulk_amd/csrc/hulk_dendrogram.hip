// hulk_dendrogram.hip — the single-linkage dendrogram of a sketch collection (hulk_dendrogram): the minimum spanning forest of the
// graph whose edge {i, j} weighs w(i, j) = fmin(d(i, j), d(j, i)), d = HULKdata.GetDistance exactly as k_smash (hulk_pairwise.hip)
// computes it with i the subject; no edge where both directions are NaN.  Edges are totally ordered by (w, lo, hi), so the forest is
// unique whatever ties; cut at any tau it is hulk_cluster's components at tau.  Boruvka's algorithm: at most ceil(log2 N) rounds, each
// ONE pass of the pair tile over the set (what k_cluster_link does) and a contraction on the host (hulk_boruvka.h).  No N x N array.
//   the set           prepared once with k_smash_prep, slot-major doubles mT / wT [slot][NP] (NP = N rounded up to 64, zero rows
//                     behind N), resident for the call as in hulk_cluster: 16 * S bytes a sketch; the raw upload is freed behind the
//                     preparation, so the PEAK of device memory is 32 * S * N bytes, or the resident set plus the scratch below,
//                     whichever is larger.  The limit on N is hulk_cluster's (HULK_CLUSTER_MAX_N)
//   comp[NP]          uint32, the identity at the start: the smallest member of a sketch's component, uploaded before every round
//   k_dendro_offer    SET::tile over one set with k_cluster_link's index arithmetic (jaccard, bottomk: the tiles on and above the diagonal,
//                     inside them s < q; weighted jaccard: the full square, s != q), once per band of band_rows subject rows.  The
//                     epilogue forms d with pair_distance; a pair inside the set, of two components, whose d is not NaN OFFERS
//                     (d, q) to s and (d, s) to q.  A sketch's best offer is the lexicographic minimum of (d bits, partner).  The
//                     tile reduces its 32 row minima over the 16 tx lanes and its 64 column minima over the 8 ty groups (shuffles
//                     that halve what a lane holds, and one LDS exchange between the two waves) and writes 32 + 64 partial offers with plain stores:
//                       row scratch  [band row][column tile]          band_rows x (NP / 64) entries
//                       col scratch  [sketch][row tile of the band]   NP x (band_rows / 32) entries
//                     of 12 bytes (the distance's bits, the partner), both sized by ONE band (band_rows at most N rounded up to
//                     32): 75 MB at N = 65,536 with the default band of 2,048.  "No offer": all ones in the distance bits.  No
//                     atomics, nothing between workgroups inside a launch: the kernel boundary is the only ordering.
//                     The zero rows behind N "agree" in every slot (d = 0): s < N && q < N masks them.  comp is allocated for NP
//   k_dendro_fold     behind every band, one wave a sketch: folds the band's partials into best[i] (the first band of a round
//                     starts from "no offer")
//   the host          downloads best (12 bytes a sketch) behind each round — the round's one synchronisation —, contracts,
//                     uploads comp (4 * N bytes); stops when one component is left or a round delivered no offer
// The output does not depend on bands, launch shape or the number of rounds: every minimum is over a total order.
#include "hulk_oneshot.h"
#include "hulk_boruvka.h"

#include <algorithm>
#include <cmath>

namespace hulk {
namespace {

constexpr uint32_t DENDRO_DEFAULT_BAND = 2048;                      // hulk_cluster's
constexpr uint32_t DENDRO_MAX_BAND = 1u << 20;                      // (band_rows / 32 is grid.y of k_dendro_offer)
constexpr uint32_t DENDRO_MAX_N = HULK_CLUSTER_MAX_N;
constexpr uint32_t NO_PARTNER = 0xFFFFFFFFu;

// (d, p) = min((d, p), (od, op)) by distance bits, then partner
__device__ __forceinline__ void offer_min(uint64_t &d, uint32_t &p, uint64_t od, uint32_t op) {
    const bool take = od < d || (od == d && op < p);
    d = take ? od : d;
    p = take ? op : p;
}

// set: the prepared set [NP rows] (mT / wT: its two buffers, SET::view).  Subjects b0 + 32 * blockIdx.y .., others 64 * (qt0 + blockIdx.x) ..; CT = NP / 64, RT = the
// pitch of the column scratch (the band's planned row tiles).  Every launched workgroup writes its 32 row and 64 column entries.
// METRIC 0 (jaccard, bottomk) is symmetric: the tiles on and above the diagonal.
// dendro_offer is the kernel's text.  It stays a function under k_dendro_offer because hipcc compiles it differently as the kernel's
// own body: the epilogue's selects become branches, 7 % more instructions
template <class SET>
__device__ __forceinline__ void dendro_offer(const SET set, uint32_t NP, uint32_t N, uint32_t b0, uint32_t qt0, uint32_t S,
                                             const uint32_t *__restrict__ comp, uint32_t RT, uint64_t *__restrict__ row_d,
                                             uint32_t *__restrict__ row_p, uint64_t *__restrict__ col_d, uint32_t *__restrict__ col_p) {
    const uint32_t ct = qt0 + blockIdx.x, CT = NP / PAIR_TQ;
    const uint32_t s0 = b0 + blockIdx.y * PAIR_TS, q0 = ct * PAIR_TQ;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;     // other quad, subject quad inside the tile
    if (SET::METRIC == 0 && s0 >= q0 + PAIR_TQ - 1) {               // jaccard: every pair of the tile has s >= q — nothing to offer
        if (tid < PAIR_TS) {
            const size_t at = (size_t)(s0 - b0 + (uint32_t)tid) * CT + ct;
            row_d[at] = BORUVKA_NONE; row_p[at] = NO_PARTNER;
        } else if (tid < PAIR_TS + PAIR_TQ) {
            const size_t at = (size_t)(q0 + (uint32_t)tid - PAIR_TS) * RT + blockIdx.y;
            col_d[at] = BORUVKA_NONE; col_p[at] = NO_PARTNER;
        }
        return;                                                     // (the whole workgroup)
    }
    __shared__ uint64_t x_d[PAIR_TQ];                               // the second wave's column minima
    __shared__ uint32_t x_p[PAIR_TQ];
    double acc[4][4], uni[4];
    uint32_t cnt[4][4];
    set.tile(s0, set, q0, S, acc, uni, cnt);
    // the epilogue: the accumulators die pair by pair into 4 row and 4 column minima
    uint32_t cs[4], cq[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { cs[i] = comp[s0 + 4 * ty + i]; cq[i] = comp[q0 + 4 * tx + i]; }      // (below NP: comp is padded)
    uint64_t rd[4], cd[4];
    uint32_t rp[4], cp[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { rd[i] = cd[i] = BORUVKA_NONE; rp[i] = cp[i] = NO_PARTNER; }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t s = s0 + 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t q = q0 + 4 * tx + j;
            const double d = pair_distance<SET::METRIC>(acc[i][j], uni[i], cnt[i][j], S);
            const bool pair = SET::METRIC == 1 ? s != q : s < q;    // (jaccard: (q, s) is this pair again, bit for bit)
            const bool ok = s < N && q < N && pair && cs[i] != cq[j] && d == d;
            const uint64_t bits = ok ? (uint64_t)__double_as_longlong(d) : BORUVKA_NONE;
            // q ascends with j and s with i: a strict compare keeps the smaller partner at equal d ("no offer" is never below)
            if (bits < rd[i]) { rd[i] = bits; rp[i] = q; }
            if (bits < cd[j]) { cd[j] = bits; cp[j] = s; }
        }
    }
    // Four minima a lane over 16 lanes, halving: a lane keeps the two of its four that its lane bit names and trades the other two
    // for its neighbour's copies of those (2 exchanges), then one of the two (1 exchange); what is left, one minimum a lane, runs a
    // plain butterfly over the remaining lane bits.  5 exchanges for the rows and 3 for the columns, where a butterfly per value
    // takes 16 and 8
    // rows: over the 16 tx lanes (consecutive lanes of one wave); the lane ends with row 2 * (tx & 1) + ((tx >> 1) & 1)
    {
        const bool hi = tx & 1, hi2 = tx & 2;
        uint64_t k0 = hi ? rd[2] : rd[0], k1 = hi ? rd[3] : rd[1];
        uint32_t p0 = hi ? rp[2] : rp[0], p1 = hi ? rp[3] : rp[1];
        offer_min(k0, p0, __shfl_xor(hi ? rd[0] : rd[2], 1), __shfl_xor(hi ? rp[0] : rp[2], 1));
        offer_min(k1, p1, __shfl_xor(hi ? rd[1] : rd[3], 1), __shfl_xor(hi ? rp[1] : rp[3], 1));
        uint64_t v = hi2 ? k1 : k0;
        uint32_t vp = hi2 ? p1 : p0;
        offer_min(v, vp, __shfl_xor(hi2 ? k0 : k1, 2), __shfl_xor(hi2 ? p0 : p1, 2));
#pragma unroll
        for (int o = 4; o < 16; o <<= 1) offer_min(v, vp, __shfl_xor(v, o), __shfl_xor(vp, o));
        if (tx < 4) {
            const uint32_t r = 2 * (tx & 1) + ((tx >> 1) & 1);
            const size_t at = (size_t)(s0 - b0 + 4 * ty + r) * CT + ct;
            row_d[at] = v; row_p[at] = vp;
        }
    }
    // columns: over the 4 ty groups of a wave (lane bits 4 and 5) — every lane of a wave ends with one of its 64 columns,
    // 4 * tx + 2 * (ty & 1) + ((ty >> 1) & 1) —, then the two waves through LDS (free behind the tile's last barrier)
    {
        const bool hi = ty & 1, hi2 = ty & 2;
        uint64_t k0 = hi ? cd[2] : cd[0], k1 = hi ? cd[3] : cd[1];
        uint32_t p0 = hi ? cp[2] : cp[0], p1 = hi ? cp[3] : cp[1];
        offer_min(k0, p0, __shfl_xor(hi ? cd[0] : cd[2], 16), __shfl_xor(hi ? cp[0] : cp[2], 16));
        offer_min(k1, p1, __shfl_xor(hi ? cd[1] : cd[3], 16), __shfl_xor(hi ? cp[1] : cp[3], 16));
        uint64_t v = hi2 ? k1 : k0;
        uint32_t vp = hi2 ? p1 : p0;
        offer_min(v, vp, __shfl_xor(hi2 ? k0 : k1, 32), __shfl_xor(hi2 ? p0 : p1, 32));
        const uint32_t c = 4 * tx + 2 * (ty & 1) + ((ty >> 1) & 1);
        if (ty >= 4) { x_d[c] = v; x_p[c] = vp; }
        __syncthreads();
        if (ty < 4) {
            offer_min(v, vp, x_d[c], x_p[c]);
            const size_t at = (size_t)(q0 + c) * RT + blockIdx.y;
            col_d[at] = v; col_p[at] = vp;
        }
    }
}

// The kernel takes mT, wT and the pitch as the dense kernels always did and builds the set here: passed as a struct the argument
// loads split and the weighted kernels measured 1 - 3.5 % slower (profiles/pairset.txt)
template <class SET>
__global__ __launch_bounds__(128) void k_dendro_offer(const double *__restrict__ mT, const double *__restrict__ wT, uint32_t NP, uint32_t N,
                                                      uint32_t b0, uint32_t qt0, uint32_t S,
                                                      const uint32_t *__restrict__ comp, uint32_t RT, uint64_t *__restrict__ row_d,
                                                      uint32_t *__restrict__ row_p, uint64_t *__restrict__ col_d, uint32_t *__restrict__ col_p) {
    dendro_offer(SET::view(mT, wT, NP, S), NP, N, b0, qt0, S, comp, RT, row_d, row_p, col_d, col_p);
}

// one wave a sketch: best[i] = min(best[i] (fresh: no offer), the band's row partials of i (if the band holds row i: the column tiles
// from qt0 on), its column partials (if i's column tile was launched: the rt row tiles of this band))
__global__ __launch_bounds__(256) void k_dendro_fold(uint32_t N, uint32_t NP, uint32_t b0, uint32_t rows, uint32_t qt0, uint32_t RT, uint32_t rt,
                                                     uint32_t fresh, const uint64_t *__restrict__ row_d, const uint32_t *__restrict__ row_p,
                                                     const uint64_t *__restrict__ col_d, const uint32_t *__restrict__ col_p,
                                                     uint64_t *__restrict__ best_d, uint32_t *__restrict__ best_p) {
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, CT = NP / PAIR_TQ;
    if (i >= N) return;                                             // (the whole wave)
    uint64_t d = BORUVKA_NONE;
    uint32_t p = NO_PARTNER;
    if (i >= b0 && i - b0 < rows)
        for (uint32_t c = qt0 + lane; c < CT; c += 64) { const size_t at = (size_t)(i - b0) * CT + c; offer_min(d, p, row_d[at], row_p[at]); }
    if (i / PAIR_TQ >= qt0)
        for (uint32_t r = lane; r < rt; r += 64) { const size_t at = (size_t)i * RT + r; offer_min(d, p, col_d[at], col_p[at]); }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) offer_min(d, p, __shfl_xor(d, o), __shfl_xor(p, o));
    if (lane == 0) {
        if (!fresh) offer_min(d, p, best_d[i], best_p[i]);
        best_d[i] = d; best_p[i] = p;
    }
}

}  // namespace
}  // namespace hulk

using namespace hulk;

extern "C" int hulk_dendrogram(int device, const uint64_t *mins, const double *weights, uint32_t n, uint32_t sketch_size,
                               const hulk_dendrogram_opts *opts, uint32_t *edge_a, uint32_t *edge_b, double *edge_distance,
                               uint32_t *n_edges, hulk_dendrogram_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_edges) *n_edges = 0;
    if (const int rc = collection_args("hulk_dendrogram", mins, weights, opts, edge_a && edge_b && edge_distance && n_edges, n, sketch_size, DENDRO_MAX_N))
        return rc;
    if (opts->band_rows % 32) return fail(nullptr, HULK_ERR_ARG, "hulk_dendrogram: band_rows must be a multiple of 32");
    if (const int rc = collection_flags("hulk_dendrogram", opts, 0)) return rc;
    const double t0 = now_s();
    if (const int rc = oneshot_device(device)) return rc;
    const uint32_t N = n, S = sketch_size, NP = smash_padded_n(N), CT = NP / PAIR_TQ;
    const uint32_t band = opts->band_rows ? std::min(opts->band_rows, DENDRO_MAX_BAND) : DENDRO_DEFAULT_BAND;
    const uint32_t bands = (uint32_t)(((uint64_t)N + band - 1) / band);
    const uint32_t band_alloc = std::min(band, (N + 31) / 32 * 32), RT = band_alloc / PAIR_TS;      // (what a band can hold of this set)
    const int metric = opts->metric;
    // experiment (tools/dendrogram_cost.py, the profiling build only): stop behind this many rounds — the forest is then incomplete
    const char *only = HULK_EXP_ENV("HULK_DENDRO_ROUNDS");
    const uint32_t max_rounds = only ? (uint32_t)atoi(only) : 0xFFFFFFFFu;
    Boruvka forest(N);
    uint32_t rounds = 0;
    double ms_offer = 0.0, ms_fold = 0.0;
    if (N > 1) {
        const size_t n_row = (size_t)band_alloc * CT, n_col = (size_t)NP * RT;
        OneShot own;                                                // events per band: before the offer kernel, behind it, behind the fold
        double *d_mT = nullptr, *d_wT = nullptr;
        uint32_t *d_comp = nullptr, *d_row_p = nullptr, *d_col_p = nullptr, *d_best_p = nullptr;
        uint64_t *d_row_d = nullptr, *d_col_d = nullptr, *d_best_d = nullptr;
        // (the peak of device memory: the header comment.  bottomk: the same buffers hold the sorted run-length form, BottomkSet::view)
        if (const int rc = prepare_set(own, metric, mins, weights, N, S, d_mT, d_wT)) return rc;
        ONESHOT_CHK(own.alloc(&d_comp, NP));
        ONESHOT_CHK(own.alloc(&d_row_d, n_row)); ONESHOT_CHK(own.alloc(&d_row_p, n_row));
        ONESHOT_CHK(own.alloc(&d_col_d, n_col)); ONESHOT_CHK(own.alloc(&d_col_p, n_col));
        ONESHOT_CHK(own.alloc(&d_best_d, N)); ONESHOT_CHK(own.alloc(&d_best_p, N));
        ONESHOT_CHK(hipMemset(d_comp, 0, (size_t)NP * 4));
        for (uint32_t e = 0; e < 3 * bands; e++) { hipEvent_t ev = nullptr; ONESHOT_CHK(own.event(&ev)); }
        const std::vector<hipEvent_t> &ev = own.events;
        std::vector<uint64_t> best_d(N);
        std::vector<uint32_t> best_p(N);
        const dim3 fg((N + 3) / 4);
        while (forest.components > 1 && rounds < max_rounds) {
            ONESHOT_CHK(hipMemcpy(d_comp, forest.comp.data(), (size_t)N * 4, hipMemcpyHostToDevice));
            // the bands of a round are queued back to back; the download of best behind them is the round's one synchronisation
            uint32_t b = 0;
            for (uint64_t b0 = 0; b0 < N; b0 += band, b++) {
                const uint32_t rows = (uint32_t)std::min<uint64_t>(band, N - b0), rt = (rows + PAIR_TS - 1) / PAIR_TS;
                // jaccard: the tiles in front of the band's first row lie below the diagonal
                const uint32_t qt0 = metric == HULK_METRIC_WEIGHTED_JACCARD ? 0u : (uint32_t)b0 / PAIR_TQ;
                const dim3 g(CT - qt0, rt);
                ONESHOT_CHK(hipEventRecord(ev[3 * b], nullptr));
                with_set(metric, d_mT, d_wT, NP, S, [&](auto set) {
                    hipLaunchKernelGGL(k_dendro_offer<decltype(set)>, g, dim3(128), 0, nullptr, d_mT, d_wT, NP, N, (uint32_t)b0, qt0, S, d_comp, RT, d_row_d, d_row_p, d_col_d, d_col_p);
                });
                ONESHOT_CHK(hipGetLastError());
                ONESHOT_CHK(hipEventRecord(ev[3 * b + 1], nullptr));
                hipLaunchKernelGGL(k_dendro_fold, fg, dim3(256), 0, nullptr, N, NP, (uint32_t)b0, rows, qt0, RT, rt, b0 == 0 ? 1u : 0u,
                                   d_row_d, d_row_p, d_col_d, d_col_p, d_best_d, d_best_p);
                ONESHOT_CHK(hipGetLastError());
                ONESHOT_CHK(hipEventRecord(ev[3 * b + 2], nullptr));
            }
            ONESHOT_CHK(hipMemcpy(best_d.data(), d_best_d, (size_t)N * 8, hipMemcpyDeviceToHost));
            ONESHOT_CHK(hipMemcpy(best_p.data(), d_best_p, (size_t)N * 4, hipMemcpyDeviceToHost));
            for (uint32_t k = 0; k < bands; k++) {
                float x = 0, y = 0;
                ONESHOT_CHK(hipEventElapsedTime(&x, ev[3 * k], ev[3 * k + 1]));
                ONESHOT_CHK(hipEventElapsedTime(&y, ev[3 * k + 1], ev[3 * k + 2]));
                ms_offer += x; ms_fold += y;
            }
            rounds++;
            const long added = forest.contract(best_d.data(), best_p.data());
            if (added < 0) return fail(nullptr, HULK_ERR_HIP, "hulk_dendrogram: an offer from outside the set or from inside a sketch's own component (corrupt device memory)");
            if (added == 0) break;                                  // what is left is separated by NaNs
        }
    }
    forest.finish();
    for (size_t e = 0; e < forest.edges.size(); e++) {
        edge_a[e] = forest.edges[e].lo; edge_b[e] = forest.edges[e].hi;
        memcpy(&edge_distance[e], &forest.edges[e].d, 8);
    }
    *n_edges = (uint32_t)forest.edges.size();
    if (stats) {
        stats->seconds_total = now_s() - t0; stats->kernel_ms_offer = ms_offer; stats->kernel_ms_fold = ms_fold;
        stats->rounds = rounds; stats->bands = bands; stats->edges = *n_edges; stats->components = forest.components;
    }
    return HULK_OK;
}
