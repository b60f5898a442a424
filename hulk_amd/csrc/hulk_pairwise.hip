// hulk_pairwise.hip — distances between sketches (HULKdata.GetDistance, sketchio.go:259-306) over prepared, slot-major sets:
//   k_smash_prep   (double)min and |w| of a set of sketches, slot-major: what every kernel below, k_search_dist (hulk_search.hip)
//                  and k_cluster_link (hulk_cluster.hip) read
//   k_smash        the N x N matrix of `hulk smash`: the pair tile's layout (hulk_pairtile.h) over one set, in a loop of its own
//   k_snap_panel   the <= 16 sketch snapshots of a flush against a resident panel (hulk_set_panel / hulk_panel_distances)
#include "hulk_device.h"
#include "hulk_pairtile.h"

#include <math.h>
#include <stdlib.h>
#include <algorithm>

namespace hulk {
namespace {

// ==========================================================================================
// hulk smash: pairwise distance matrix over N sketches of S slots.
// distances.GetDistance "jaccard" (distances.go:19-26) and GetWJD (distances.go:44-72) with the
// reference's quirk that BOTH weight vectors come from the subject sketch (sketchio.go:293-301).
// Every pair (s, q) accumulates over the slots IN ORDER, so the fp64 sums are bit-identical to the Go loops.
//   k_smash_prep  once per call: mins -> float64 (the reference compares them as float64, sketchio.go:271-277), weights ->
//                 |w| (max(max(w,0), max(-w,0)), NaN stays NaN), both stored SLOT-major ([slot][sketch]) so that a tile's rows
//                 are contiguous
//   k_smash       the register tile whose layout and contract hulk_pairtile.h writes down (32 subjects x 64 queries a workgroup,
//                 chunks of 32 slots double-buffered through LDS, 16 accumulators a thread adding in slot order) over one set,
//                 both sides the same arrays; every pair with both sketches below N is stored.  The loop is k_smash's OWN copy of
//                 pair_tile's: the header says why (1.1 % of the weighted kernel) and what keeps the two in step
// ==========================================================================================
__global__ __launch_bounds__(256) void k_smash_prep(const unsigned long long *__restrict__ mins, const double *__restrict__ weights,
                                                    uint32_t N, uint32_t S, uint32_t NP, double *__restrict__ mT, double *__restrict__ wT) {
    // 32 x 32 tiles through LDS: reads run along the slots of a sketch, writes along the sketches of a slot
    __shared__ double tm[32][33], tw[32][33];
    const uint32_t n0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (uint32_t r = ty; r < 32; r += 8) {
        const uint32_t n = n0 + r, c = c0 + tx;
        const bool ok = n < N && c < S;
        tm[r][tx] = ok ? (double)mins[(size_t)n * S + c] : 0.0;
        tw[r][tx] = ok ? fabs(weights[(size_t)n * S + c]) : 0.0;
    }
    __syncthreads();
    for (uint32_t r = ty; r < 32; r += 8) {
        const uint32_t c = c0 + r, n = n0 + tx;
        if (c < S && n < NP) { mT[(size_t)c * NP + n] = tm[tx][r]; wT[(size_t)c * NP + n] = tw[tx][r]; }
    }
}

template <int METRIC>
__global__ __launch_bounds__(128) void k_smash(const double *__restrict__ mT, const double *__restrict__ wT, uint32_t N, uint32_t NP,
                                               uint32_t S, double *__restrict__ out) {
    __shared__ __align__(16) double ma[2][PAIR_CH][PAIR_TS + PAIR_PAD], wa[2][PAIR_CH][PAIR_TS + PAIR_PAD];
    __shared__ __align__(16) double mb[2][PAIR_CH][PAIR_TQ + PAIR_PAD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;     // query quad, subject quad inside the tile
    const uint32_t s0 = blockIdx.y * PAIR_TS, q0 = blockIdx.x * PAIR_TQ;
    // staging: thread t moves slot (t / 4) of the chunk: 8 subject rows (mins, weights) and 16 query rows from (t % 4) on
    const int lc = tid >> 2, lr = tid & 3;
    double acc[4][4], uni[4];
    uint32_t cnt[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uni[i] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) { acc[i][j] = 0.0; cnt[i][j] = 0; }
    }
    double2 ra[4], rw[4], rb[8];
    auto fetch = [&](uint32_t c0) {
        const uint32_t col = c0 + (uint32_t)lc;
        const bool ok = col < S;                                    // (rows past N hold zeros: NP is N rounded up to the tile)
        const double2 *pa = (const double2 *)(mT + (size_t)col * NP + s0 + 8 * lr);
        const double2 *pw = (const double2 *)(wT + (size_t)col * NP + s0 + 8 * lr);
        const double2 *pb = (const double2 *)(mT + (size_t)col * NP + q0 + 16 * lr);
#pragma unroll
        for (int x = 0; x < 4; x++) { ra[x] = ok ? pa[x] : make_double2(0.0, 0.0); if (METRIC == 1) rw[x] = ok ? pw[x] : make_double2(0.0, 0.0); }
#pragma unroll
        for (int x = 0; x < 8; x++) rb[x] = ok ? pb[x] : make_double2(0.0, 0.0);
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int x = 0; x < 4; x++) { *(double2 *)&ma[buf][lc][8 * lr + 2 * x] = ra[x]; if (METRIC == 1) *(double2 *)&wa[buf][lc][8 * lr + 2 * x] = rw[x]; }
#pragma unroll
        for (int x = 0; x < 8; x++) *(double2 *)&mb[buf][lc][16 * lr + 2 * x] = rb[x];
    };
    fetch(0);
    stash(0);
    __syncthreads();
    int buf = 0;
    for (uint32_t c0 = 0; c0 < S; c0 += PAIR_CH, buf ^= 1) {
        const bool more = c0 + PAIR_CH < S;
        if (more) fetch(c0 + PAIR_CH);                             // in flight under this chunk's arithmetic
        const uint32_t lim = S - c0 < (uint32_t)PAIR_CH ? S - c0 : (uint32_t)PAIR_CH;
#pragma unroll 2
        for (uint32_t c = 0; c < lim; c++) {                       // (unrolled by two: the next slot's six LDS reads are in flight under this one's 72 VALU)
            const double2 a01 = *(const double2 *)&ma[buf][c][4 * ty], a23 = *(const double2 *)&ma[buf][c][4 * ty + 2];
            const double2 b01 = *(const double2 *)&mb[buf][c][4 * tx], b23 = *(const double2 *)&mb[buf][c][4 * tx + 2];
            const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
            if (METRIC == 1) {
                const double2 w01 = *(const double2 *)&wa[buf][c][4 * ty], w23 = *(const double2 *)&wa[buf][c][4 * ty + 2];
                const double w[4] = {w01.x, w01.y, w23.x, w23.y};
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    uni[i] += w[i];
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
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t s = s0 + 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t q = q0 + 4 * tx + j;
            if (s < N && q < N) out[(size_t)s * N + q] = pair_distance<METRIC>(acc[i][j], uni[i], cnt[i][j], S);
        }
    }
}

// ==========================================================================================
// k_snap_panel (hulk_set_panel / hulk_panel_distances): the M <= 16 sketch snapshots one flush has just recorded against a
// device-resident panel of P sketches — HULKdata.GetDistance as k_smash computes it, for a skinny M x P block.
//   the panel       slot-major doubles pmT / pwT [slot][PP] (k_smash_prep's layout: (double)min and |w|, zero rows behind P;
//                   PP = P rounded up to 64), prepared once when the panel is set
//   one lane        owns one panel sketch and MT of the flush's snapshots: it walks the slots in ascending order — the fp64
//                   sums are the Go loop's, bit for bit — with one accumulator per snapshot in registers; a panel value is
//                   loaded once per slot (consecutive lanes, consecutive addresses) and serves the MT snapshots
//   a workgroup     is ONE wave: 64 panel sketches (blockIdx.x) x MT = 4 snapshots (blockIdx.y), so a flush of 16 snapshots
//                   against P = 1024 is 64 workgroups on 64 CUs.  A wave alone on its SIMD hides no latency by itself: the
//                   panel values of the NEXT chunk of PANEL_CH slots are loaded into registers before this chunk is computed
//                   (one memory latency per 32 slots, under 32 x MT compare-and-add steps), and so are the snapshot values
//   the snapshots   entries (base + m) % cap of the ring [cap][S] (they may wrap inside one flush), staged per chunk into
//                   LDS as (double)min and |w|, two buffers, one barrier per chunk; every lane reads the same LDS address
//   ROLE row        the snapshot is the subject: its |w| is added where the mins agree, the union is the sum of its |w|
//   ROLE column     the panel sketch is the subject: the same with the panel's |w| (for jaccard the two are one kernel)
// The distances equal hulk_smash's bit for bit; where the weighted quotient is 0 / 0 or Inf / Inf, the NaN carries the sign bit
// of the amd64 division's default NaN (see the epilogue), so that the uint64 view equals the host restatement's too.
// out[(base + m) % cap][P].  MT = 1 when the flush holds a single snapshot.
// ==========================================================================================
constexpr int PANEL_CH = 32, PANEL_PAD = 2, PANEL_MT = 4;
template <int METRIC, int COLUMN, int MT>
__global__ __launch_bounds__(64) void k_snap_panel(const unsigned long long *__restrict__ snap_mins,
                                                   const double *__restrict__ snap_weights, uint32_t S, uint32_t base,
                                                   uint32_t cap, uint32_t M, const double *__restrict__ pmT,
                                                   const double *__restrict__ pwT, uint32_t P, uint32_t PP,
                                                   double *__restrict__ out) {
    __shared__ __align__(16) double sm[2][PANEL_CH][MT + PANEL_PAD], sw[2][PANEL_CH][MT + PANEL_PAD];
    constexpr bool ROW_W = METRIC == 1 && !COLUMN, COL_W = METRIC == 1 && COLUMN;
    constexpr int NST = (PANEL_CH * MT + 63) / 64;                  // snapshot values a lane stages per chunk
    const uint32_t tid = threadIdx.x, p = blockIdx.x * 64 + tid;    // (p < PP: gridDim.x is PP / 64)
    const uint32_t m0 = blockIdx.y * MT;                            // this wave's snapshots: m0 .. m0 + MT - 1 (those < M)
    double acc[MT], uni[MT];
    uint32_t cnt[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) { acc[m] = 0.0; uni[m] = 0.0; cnt[m] = 0; }
    double pv[PANEL_CH], pn[PANEL_CH], qv[COL_W ? PANEL_CH : 1], qn[COL_W ? PANEL_CH : 1], rw[NST];
    unsigned long long rm[NST];
    // chunk c0 -> registers.  Nothing here waits for a load (the conversions are stash's), and nothing branches: a slot past the end
    // of the sketch or a snapshot past M is read from the last valid one instead — the slot loop stops at `lim`, the epilogue at M
    auto fetch = [&](uint32_t c0) {
#pragma unroll
        for (int x = 0; x < NST; x++) {
            const uint32_t i = tid + 64u * x, c = min(c0 + i % PANEL_CH, S - 1), m = min(m0 + i / PANEL_CH, M - 1);
            const size_t at = (size_t)((base + m) % cap) * S + c;
            rm[x] = snap_mins[at];
            if (ROW_W) rw[x] = snap_weights[at];
        }
#pragma unroll
        for (int c = 0; c < PANEL_CH; c++) {
            const size_t at = (size_t)min(c0 + (uint32_t)c, S - 1) * PP + p;
            pn[c] = pmT[at];
            if (COL_W) qn[c] = pwT[at];
        }
    };
    auto stash = [&](int buf) {                                     // ... -> the LDS buffer nobody reads, and the current registers
#pragma unroll
        for (int x = 0; x < NST; x++) {
            const uint32_t i = tid + 64u * x, c = i % PANEL_CH, m = i / PANEL_CH;
            if (i < (uint32_t)(PANEL_CH * MT)) { sm[buf][c][m] = (double)rm[x]; if (ROW_W) sw[buf][c][m] = fabs(rw[x]); }
        }
#pragma unroll
        for (int c = 0; c < PANEL_CH; c++) { pv[c] = pn[c]; if (COL_W) qv[c] = qn[c]; }
    };
    fetch(0);
    stash(0);
    __syncthreads();
    int buf = 0;
    for (uint32_t c0 = 0; c0 < S; c0 += PANEL_CH, buf ^= 1) {
        const bool more = c0 + PANEL_CH < S;
        if (more) fetch(c0 + PANEL_CH);                             // in flight under this chunk's arithmetic
        const uint32_t lim = S - c0 < (uint32_t)PANEL_CH ? S - c0 : (uint32_t)PANEL_CH;
#pragma unroll
        for (int c = 0; c < PANEL_CH; c++) {
            if ((uint32_t)c >= lim) continue;                       // (uniform: the last chunk of a sketch may be partial)
            const double pm = pv[c];
            if (COL_W) {
                const double pw = qv[c];
                uni[0] += pw;                                       // the subject's |w|, whatever the query
#pragma unroll
                for (int m = 0; m < MT; m++) acc[m] += (pm == sm[buf][c][m]) ? pw : 0.0;
            } else if (ROW_W) {
#pragma unroll
                for (int m = 0; m < MT; m++) { const double w = sw[buf][c][m]; uni[m] += w; acc[m] += (sm[buf][c][m] == pm) ? w : 0.0; }
            } else {
#pragma unroll
                for (int m = 0; m < MT; m++) cnt[m] += (sm[buf][c][m] == pm) ? 1u : 0u;    // a count of 1.0s is exact in fp64
            }
        }
        if (more) stash(buf ^ 1);
        __syncthreads();
    }
    if (p >= P) return;
#pragma unroll
    for (int m = 0; m < MT; m++) {
        if (m0 + (uint32_t)m >= M) continue;
        double d;
        if (METRIC == 1) {
            const double a = acc[m], u = uni[COLUMN ? 0 : m], q = a / u;
            d = 1 - q;
            // 0 / 0 (weights of zeros only) and Inf / Inf (MaxFloat64 weights, the union overflows): the NaN the reference's
            // division gives on the amd64 hosts it runs on has the sign bit set (the x86 default NaN) and 1 - NaN keeps it; the
            // GPU's division gives the same NaN without the sign.  A NaN that came in with the weights goes through as it is:
            // 1 - NaN is that NaN on the host, while the subtraction here, an add of the negated operand, would turn its sign.
            if (q != q) d = (a == a && u == u) ? __longlong_as_double((long long)0xFFF8000000000000ull) : q;
        } else {
            d = 1.0 - ((double)cnt[m] / (double)S);
        }
        out[(size_t)((base + m0 + m) % cap) * P + p] = d;
    }
}

}  // namespace

// sketches rounded up to the query tile: the slot-major arrays are [S][smash_padded_n(N)], zero rows behind N
uint32_t smash_padded_n(uint32_t N) { return (N + PAIR_TQ - 1) / PAIR_TQ * PAIR_TQ; }
hipError_t launch_smash(hipStream_t s, const unsigned long long *d_mins, const double *d_weights, uint32_t N, uint32_t S,
                        int metric, double *d_out, double *d_mT, double *d_wT) {
    if (N == 0) return hipSuccess;
    const uint32_t NP = smash_padded_n(N);
    hipLaunchKernelGGL(k_smash_prep, dim3((S + 31) / 32, NP / 32), dim3(256), 0, s, d_mins, d_weights, N, S, NP, d_mT, d_wT);
    const dim3 g(NP / PAIR_TQ, (N + PAIR_TS - 1) / PAIR_TS);
    if (metric == 1) hipLaunchKernelGGL(k_smash<1>, g, dim3(128), 0, s, d_mT, d_wT, N, NP, S, d_out);
    else hipLaunchKernelGGL(k_smash<0>, g, dim3(128), 0, s, d_mT, d_wT, N, NP, S, d_out);
    return hipGetLastError();
}

// the panel of hulk_set_panel as k_snap_panel reads it: d_pmT, d_pwT [S][smash_padded_n(P)]
hipError_t launch_panel_prep(hipStream_t s, const unsigned long long *d_mins, const double *d_weights, uint32_t P, uint32_t S,
                             double *d_pmT, double *d_pwT) {
    if (P == 0 || S == 0) return hipSuccess;
    const uint32_t PP = smash_padded_n(P);
    hipLaunchKernelGGL(k_smash_prep, dim3((S + 31) / 32, PP / 32), dim3(256), 0, s, d_mins, d_weights, P, S, PP, d_pmT, d_pwT);
    return hipGetLastError();
}

template <int METRIC, int COLUMN>
static void snap_panel_mt(hipStream_t s, const unsigned long long *d_snap_mins, const double *d_snap_weights, uint32_t S,
                          uint32_t base, uint32_t cap, uint32_t M, const double *d_pmT, const double *d_pwT, uint32_t P,
                          uint32_t PP, double *d_out) {
    if (M <= 1) hipLaunchKernelGGL((k_snap_panel<METRIC, COLUMN, 1>), dim3(PP / 64, 1), dim3(64), 0, s, d_snap_mins, d_snap_weights, S, base, cap, M, d_pmT, d_pwT, P, PP, d_out);
    else hipLaunchKernelGGL((k_snap_panel<METRIC, COLUMN, PANEL_MT>), dim3(PP / 64, (M + PANEL_MT - 1) / PANEL_MT), dim3(64), 0, s, d_snap_mins, d_snap_weights, S, base, cap, M, d_pmT, d_pwT, P, PP, d_out);
}

// snapshots in entries (base + m) % cap, m < M <= SCAN_BATCH_MAX, of the ring [cap][S] against the prepared panel;
// d_out [cap][P], the same entries.  role: 0 the snapshot is the subject (its row), 1 the panel sketch is (its column)
hipError_t launch_snap_panel(hipStream_t s, const unsigned long long *d_snap_mins, const double *d_snap_weights, uint32_t S,
                             uint32_t base, uint32_t cap, uint32_t M, const double *d_pmT, const double *d_pwT, uint32_t P,
                             int metric, int role, double *d_out) {
    if (M == 0 || P == 0 || S == 0 || cap == 0) return hipSuccess;
    if (M > (uint32_t)SCAN_BATCH_MAX) return hipErrorInvalidValue;
    const uint32_t PP = smash_padded_n(P);
    static_assert(PAIR_TQ % 64 == 0, "the panel is padded to whole waves");
    prof_mark(s, "k_snap_panel");
    if (metric != 1) snap_panel_mt<0, 0>(s, d_snap_mins, d_snap_weights, S, base, cap, M, d_pmT, d_pwT, P, PP, d_out);
    else if (role == 1) snap_panel_mt<1, 1>(s, d_snap_mins, d_snap_weights, S, base, cap, M, d_pmT, d_pwT, P, PP, d_out);
    else snap_panel_mt<1, 0>(s, d_snap_mins, d_snap_weights, S, base, cap, M, d_pmT, d_pwT, P, PP, d_out);
    return hipGetLastError();
}

}  // namespace hulk
