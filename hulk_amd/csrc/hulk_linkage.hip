// hulk_linkage.hip — the single-, complete- and average-linkage dendrogram of a sketch collection (hulk_linkage): the primitive
// agglomeration over W[i][j] = fmin(d(i, j), d(j, i)), d = HULKdata.GetDistance exactly as k_smash (hulk_pairwise.hip) computes it with
// i the subject; a pair whose two directions are NaN has W = +inf and never merges.  Clusters are named by their smallest member; while
// some pair of live clusters is at a finite distance the pair (p, q), p < q, smallest under the key (d(p, q), p, q) merges into p, and
// for every other live k
//   single    d(p, k) = min(d(p, k), d(q, k))
//   complete  d(p, k) = max(d(p, k), d(q, k))
//   average   d(p, k) = (n_p * d(p, k) + n_q * d(q, k)) / (n_p + n_q), the sizes before the merge, every operation rounded on its own
// W >= 0 or +inf: a double that orders like its bits, which is how every key below is compared.
//   the matrix        launch_smash / launch_bottomk_smash fill D [N][N] on the device as hulk_smash does; k_linkage_sym turns it into W
//                     in place (32 x 32 tiles and their mirror images through LDS; the diagonal and double-NaN pairs +inf).  Full square
//                     storage, 8 * N * N bytes, kept symmetric by every merge: row p is what a merge reads, row i from i + 1 on what a
//                     rescan reads, both along consecutive addresses.  The raw upload and the prepared set are freed behind this phase
//   the cache         per row i the nearest live j > i: (nnd[i], nn[i]) = min over live j > i of (W[i][j], j); "none" is (+inf, NONE).
//                     min over i of (nnd[i], i, nn[i]) is then the smallest key (d(p, q), p, q) of all live pairs — ties included,
//                     because the cache and the pick compare the very key of the definition
//   a merge           three launches of fixed shape, ordered by the kernel boundary alone:
//     k_linkage_pick    one workgroup: the argmin of the N cached keys; writes merge t, the sizes, live[q] = 0 and (p, q, n_p, n_q) into
//                       the state; nothing finite left: state.finished = 1, and every later launch of the call returns at once
//     k_linkage_update  a thread per k: the new d(p, k) into W[p][k] and W[k][p]; q retires; a row k < q whose cached neighbour was
//                       p or q is FLAGGED, as row p is; a row k < p whose neighbour stays is offered (d(p, k), p) — the one entry
//                       of its row that changed
//     k_linkage_rescan  a workgroup per group of 16 rows: reads the group's flags in one load and rescans the flagged rows
//   the host          queues chunks of LINK_CHUNK merges back to back — p, q and "finished" never leave the device — and reads the state
//                     behind each chunk: the one synchronisation per chunk, to stop early on a forest
// Plain stores and wave reductions: no atomics, no workgroup waits for another.  The output is a function of the inputs alone.
#include "hulk_oneshot.h"

#include <algorithm>
#include <cmath>

namespace hulk {
namespace {

constexpr uint32_t LINK_MAX_N = HULK_LINKAGE_MAX_N;
constexpr uint32_t LINK_CHUNK = 4096;                               // merges between two looks at "finished"
constexpr uint32_t LINK_GROUP = 16;                                 // rows per workgroup of k_linkage_rescan
constexpr uint32_t LINK_PICK_THREADS = 1024, LINK_SCAN_THREADS = 256;
constexpr uint64_t LINK_INF = 0x7FF0000000000000ull;                // +inf
constexpr uint64_t LINK_WORST = 0xFFFFFFFFFFFFFFFFull;              // above every key
constexpr uint32_t LINK_NONE = 0xFFFFFFFFu;

struct LinkState {
    uint32_t p, q;                                                  // the merge k_linkage_pick chose
    uint32_t finished;                                              // 1: no finite pair is left; 2: a cached neighbour outside the set
    uint32_t merges;
    double np, nq;                                                  // the sizes of p and q before the merge
};

// (d, j) = min((d, j), (od, oj)) by distance bits, then index
__device__ __forceinline__ void key_min(uint64_t &d, uint32_t &j, uint64_t od, uint32_t oj) {
    const bool take = od < d || (od == d && oj < j);
    d = take ? od : d;
    j = take ? oj : j;
}

// the minimum of the workgroup's keys in every thread; xd / xj: one entry per wave
template <int WAVES>
__device__ __forceinline__ void key_min_block(uint64_t &d, uint32_t &j, uint64_t *xd, uint32_t *xj) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) key_min(d, j, __shfl_xor(d, o), __shfl_xor(j, o));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                                // (the previous round's readers are done with xd / xj)
    if (lane == 0) { xd[wave] = d; xj[wave] = j; }
    __syncthreads();
    d = xd[0]; j = xj[0];
#pragma unroll
    for (int w = 1; w < WAVES; w++) key_min(d, j, xd[w], xj[w]);
}

// D -> W in place.  Workgroup (bx, by), bx >= by, owns tile A (rows 32 * by .., columns 32 * bx ..) and its mirror image B
__global__ __launch_bounds__(256) void k_linkage_sym(double *__restrict__ W, uint32_t N) {
    const uint32_t bx = blockIdx.x, by = blockIdx.y;
    if (bx < by) return;                                            // (the whole workgroup)
    __shared__ double ta[32][33], tb[32][33];
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (uint32_t r = ty; r < 32; r += 8) {
        const uint32_t ia = by * 32 + r, ja = bx * 32 + tx, ib = bx * 32 + r, jb = by * 32 + tx;
        ta[r][tx] = (ia < N && ja < N) ? W[(size_t)ia * N + ja] : 0.0;
        tb[r][tx] = (ib < N && jb < N) ? W[(size_t)ib * N + jb] : 0.0;
    }
    __syncthreads();
    const double inf = __longlong_as_double((long long)LINK_INF);
    for (uint32_t r = ty; r < 32; r += 8) {
        const uint32_t ia = by * 32 + r, ja = bx * 32 + tx, ib = bx * 32 + r, jb = by * 32 + tx;
        double wa = fmin(ta[r][tx], tb[tx][r]), wb = fmin(tb[r][tx], ta[tx][r]);
        if (wa != wa || ia == ja) wa = inf;
        if (wb != wb || ib == jb) wb = inf;
        if (ia < N && ja < N) W[(size_t)ia * N + ja] = wa;
        if (bx != by && ib < N && jb < N) W[(size_t)ib * N + jb] = wb;
    }
}

__global__ __launch_bounds__(256) void k_linkage_init(uint32_t N, uint64_t *__restrict__ nnd, uint32_t *__restrict__ nn, uint32_t *__restrict__ size,
                                                      uint8_t *__restrict__ live, uint8_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    nnd[i] = LINK_INF; nn[i] = LINK_NONE; size[i] = 1; live[i] = 1; flag[i] = 1;
}

// merge t: the smallest (nnd[i], i) — nn[i] is the smallest j of that distance already
__global__ __launch_bounds__(LINK_PICK_THREADS) void k_linkage_pick(uint32_t t, uint32_t N, const uint64_t *__restrict__ nnd, const uint32_t *__restrict__ nn,
                                                                    uint32_t *__restrict__ size, uint8_t *__restrict__ live, LinkState *__restrict__ st,
                                                                    uint32_t *__restrict__ merge_a, uint32_t *__restrict__ merge_b,
                                                                    uint64_t *__restrict__ merge_d, uint32_t *__restrict__ merge_size) {
    __shared__ uint64_t xd[LINK_PICK_THREADS / 64];
    __shared__ uint32_t xj[LINK_PICK_THREADS / 64];
    if (st->finished) return;                                       // (the whole workgroup)
    uint64_t d = LINK_WORST;
    uint32_t p = LINK_NONE;
    for (uint32_t i = threadIdx.x; i < N; i += LINK_PICK_THREADS) {
        const uint64_t x = nnd[i];
        if (x < d) { d = x; p = i; }                                // (i ascends: the smaller row stays at equal distance)
    }
    key_min_block<LINK_PICK_THREADS / 64>(d, p, xd, xj);
    if (threadIdx.x != 0) return;
    if (d >= LINK_INF) { st->finished = 1; return; }
    const uint32_t q = nn[p];
    if (q >= N || q <= p || !live[p] || !live[q]) { st->finished = 2; return; }
    const uint32_t np = size[p], nq = size[q];
    merge_a[t] = p; merge_b[t] = q; merge_d[t] = d; merge_size[t] = np + nq;
    size[p] = np + nq;
    live[q] = 0;
    st->p = p; st->q = q; st->np = (double)np; st->nq = (double)nq; st->merges = t + 1;
}

// the distance of the union p + q to k from a = d(p, k) and b = d(q, k)
__device__ __forceinline__ double linkage_distance(int method, double a, double b, double np, double nq) {
#pragma clang fp contract(off)
    if (method == HULK_LINKAGE_SINGLE) return fmin(a, b);
    if (method == HULK_LINKAGE_COMPLETE) return fmax(a, b);
    return __ddiv_rn(__dadd_rn(__dmul_rn(np, a), __dmul_rn(nq, b)), __dadd_rn(np, nq));
}

__global__ __launch_bounds__(256) void k_linkage_update(uint32_t N, int method, double *__restrict__ W, uint64_t *__restrict__ nnd, uint32_t *__restrict__ nn,
                                                        const uint8_t *__restrict__ live, uint8_t *__restrict__ flag, const LinkState *__restrict__ st) {
    if (st->finished) return;
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= N) return;
    const uint32_t p = st->p, q = st->q;                            // (p < q < N: k_linkage_pick checked)
    if (k == q) { nnd[q] = LINK_INF; nn[q] = LINK_NONE; flag[q] = 0; return; }
    if (k == p) { flag[p] = 1; return; }
    if (!live[k]) return;
    const double d = linkage_distance(method, W[(size_t)p * N + k], W[(size_t)q * N + k], st->np, st->nq);
    W[(size_t)p * N + k] = d;
    W[(size_t)k * N + p] = d;
    if (k > q) return;                                              // (its row looks at j > k only: neither p nor q)
    const uint32_t c = nn[k];
    if (c == q || c == p) { flag[k] = 1; return; }                  // (k > p: c is never p)
    if (k > p) return;
    const uint64_t bits = (uint64_t)__double_as_longlong(d), old = nnd[k];
    if (bits < LINK_INF && (bits < old || (bits == old && p < c))) { nnd[k] = bits; nn[k] = p; }
}

// workgroup b: the flagged rows among b * LINK_GROUP ..; row i: (nnd, nn) = the minimum of (W[i][j], j) over the live j > i
__global__ __launch_bounds__(LINK_SCAN_THREADS) void k_linkage_rescan(uint32_t N, const double *__restrict__ W, const uint8_t *__restrict__ live,
                                                                      uint64_t *__restrict__ nnd, uint32_t *__restrict__ nn, uint8_t *__restrict__ flag,
                                                                      const LinkState *__restrict__ st, uint32_t *__restrict__ rescanned) {
    __shared__ uint64_t xd[LINK_SCAN_THREADS / 64];
    __shared__ uint32_t xj[LINK_SCAN_THREADS / 64];
    __shared__ uint32_t todo;
    if (st->finished) return;                                       // (the whole workgroup)
    const uint32_t r0 = blockIdx.x * LINK_GROUP, tid = threadIdx.x;
    if (tid < 64) {
        const uint32_t i = r0 + tid;
        const bool f = tid < LINK_GROUP && i < N && flag[i] != 0;
        const unsigned long long m = __ballot(f);
        if (tid == 0) todo = (uint32_t)m;
    }
    __syncthreads();
    uint32_t m = todo, done = 0;                                    // (uniform)
    while (m) {
        const uint32_t i = r0 + (uint32_t)__builtin_ctz(m);
        m &= m - 1;
        const uint64_t *row = (const uint64_t *)W + (size_t)i * N;
        uint64_t d = LINK_WORST;
        uint32_t j0 = LINK_NONE;
#pragma unroll 4
        for (uint32_t j = i + 1 + tid; j < N; j += LINK_SCAN_THREADS) {
            const uint64_t w = row[j];                              // (both loads issue at once: neither waits for the other)
            const uint64_t x = live[j] ? w : LINK_WORST;
            if (x < d) { d = x; j0 = j; }                           // (j ascends: the smaller column stays at equal distance)
        }
        key_min_block<LINK_SCAN_THREADS / 64>(d, j0, xd, xj);
        if (tid == 0) {
            const bool none = d >= LINK_INF;
            nnd[i] = none ? LINK_INF : d; nn[i] = none ? LINK_NONE : j0; flag[i] = 0;
        }
        done++;
    }
    if (tid == 0 && done) rescanned[blockIdx.x] += done;            // (this workgroup's own counter: the host adds them up)
}

}  // namespace
}  // namespace hulk

using namespace hulk;

extern "C" int hulk_linkage(int device, const uint64_t *mins, const double *weights, uint32_t n, uint32_t sketch_size,
                            const hulk_linkage_opts *opts, uint32_t *merge_a, uint32_t *merge_b, double *merge_distance,
                            uint32_t *merge_size, uint32_t *n_merges, hulk_linkage_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_merges) *n_merges = 0;
    if (const int rc = collection_args("hulk_linkage", mins, weights, opts, merge_a && merge_b && merge_distance && merge_size && n_merges, n,
                                       sketch_size, LINK_MAX_N))
        return rc;
    if (opts->method != HULK_LINKAGE_SINGLE && opts->method != HULK_LINKAGE_COMPLETE && opts->method != HULK_LINKAGE_AVERAGE)
        return fail(nullptr, HULK_ERR_ARG, "hulk_linkage: method");
    if (const int rc = collection_flags("hulk_linkage", opts, 0)) return rc;
    const double t0 = now_s();
    if (const int rc = oneshot_device(device)) return rc;
    const uint32_t N = n, S = sketch_size, NP = smash_padded_n(N);
    const int metric = opts->metric, method = opts->method;
    const bool bottomk = metric == HULK_METRIC_BOTTOMK;             // (reads no weights: they may be NULL)
    uint32_t merges = 0;
    uint64_t rescans = 0;
    double ms_matrix = 0.0, ms_merge = 0.0;
    if (N > 1) {
        const size_t NS = (size_t)N * S, NT = (size_t)NP * S, NN = (size_t)N * N;
        {
            // the peak is the matrix phase: the matrix, the raw upload and the prepared set
            size_t free_b = 0, total_b = 0;
            ONESHOT_CHK(hipMemGetInfo(&free_b, &total_b));
            const size_t need = NN * 8 + NS * 16 + NT * 16 + (size_t)N * 64 + (1u << 20);
            if (need > free_b)
                return fail(nullptr, HULK_ERR_HIP, "hulk_linkage: out of device memory: the n x n matrix of " + std::to_string(N) + " sketches and the set need " +
                                                   std::to_string(need) + " bytes, " + std::to_string(free_b) + " are free");
        }
        OneShot own;
        unsigned long long *d_raw_m = nullptr; double *d_raw_w = nullptr, *d_mT = nullptr, *d_wT = nullptr, *d_W = nullptr;
        hipEvent_t ev[4];
        for (hipEvent_t &e : ev) ONESHOT_CHK(own.event(&e));
        ONESHOT_CHK(own.alloc(&d_W, NN));
        ONESHOT_CHK(own.alloc(&d_mT, NT)); ONESHOT_CHK(own.alloc(&d_wT, NT));
        ONESHOT_CHK(own.alloc(&d_raw_m, NS)); ONESHOT_CHK(own.alloc(&d_raw_w, NS));
        ONESHOT_CHK(hipMemcpy(d_raw_m, mins, NS * 8, hipMemcpyHostToDevice));
        if (!bottomk) ONESHOT_CHK(hipMemcpy(d_raw_w, weights, NS * 8, hipMemcpyHostToDevice));
        ONESHOT_CHK(hipEventRecord(ev[0], nullptr));
        if (bottomk) ONESHOT_CHK(launch_bottomk_smash(nullptr, d_raw_m, N, S, d_W, d_mT, d_wT));
        else ONESHOT_CHK(launch_smash(nullptr, d_raw_m, d_raw_w, N, S, metric, d_W, d_mT, d_wT));
        const uint32_t T = (N + 31) / 32;
        hipLaunchKernelGGL(k_linkage_sym, dim3(T, T), dim3(256), 0, nullptr, d_W, N);
        ONESHOT_CHK(hipGetLastError());
        ONESHOT_CHK(hipEventRecord(ev[1], nullptr));
        ONESHOT_CHK(hipDeviceSynchronize());
        ONESHOT_CHK(own.release(d_raw_m)); ONESHOT_CHK(own.release(d_raw_w));
        ONESHOT_CHK(own.release(d_mT)); ONESHOT_CHK(own.release(d_wT));
        const uint32_t groups = (N + LINK_GROUP - 1) / LINK_GROUP, blocks = (N + 255) / 256;
        uint64_t *d_nnd = nullptr, *d_md = nullptr;
        uint32_t *d_nn = nullptr, *d_size = nullptr, *d_ma = nullptr, *d_mb = nullptr, *d_ms = nullptr, *d_rescanned = nullptr;
        uint8_t *d_live = nullptr, *d_flag = nullptr;
        LinkState *d_st = nullptr;
        ONESHOT_CHK(own.alloc(&d_nnd, N)); ONESHOT_CHK(own.alloc(&d_nn, N)); ONESHOT_CHK(own.alloc(&d_size, N));
        ONESHOT_CHK(own.alloc(&d_live, N)); ONESHOT_CHK(own.alloc(&d_flag, N));
        ONESHOT_CHK(own.alloc(&d_ma, N)); ONESHOT_CHK(own.alloc(&d_mb, N)); ONESHOT_CHK(own.alloc(&d_md, N)); ONESHOT_CHK(own.alloc(&d_ms, N));
        ONESHOT_CHK(own.alloc(&d_rescanned, groups)); ONESHOT_CHK(own.alloc(&d_st, 1));
        ONESHOT_CHK(hipMemsetAsync(d_st, 0, sizeof(LinkState), nullptr));
        ONESHOT_CHK(hipMemsetAsync(d_rescanned, 0, (size_t)groups * 4, nullptr));
        hipLaunchKernelGGL(k_linkage_init, dim3(blocks), dim3(256), 0, nullptr, N, d_nnd, d_nn, d_size, d_live, d_flag);
        ONESHOT_CHK(hipGetLastError());
        ONESHOT_CHK(hipEventRecord(ev[2], nullptr));
        // every row is flagged: the first rescan fills the cache
        hipLaunchKernelGGL(k_linkage_rescan, dim3(groups), dim3(LINK_SCAN_THREADS), 0, nullptr, N, d_W, d_live, d_nnd, d_nn, d_flag, d_st, d_rescanned);
        ONESHOT_CHK(hipGetLastError());
        LinkState st;
        memset(&st, 0, sizeof st);
        for (uint32_t t = 0; t < N - 1 && !st.finished;) {
            const uint32_t end = (uint32_t)std::min<uint64_t>((uint64_t)t + LINK_CHUNK, N - 1);
            for (; t < end; t++) {
                hipLaunchKernelGGL(k_linkage_pick, dim3(1), dim3(LINK_PICK_THREADS), 0, nullptr, t, N, d_nnd, d_nn, d_size, d_live, d_st, d_ma, d_mb, d_md, d_ms);
                hipLaunchKernelGGL(k_linkage_update, dim3(blocks), dim3(256), 0, nullptr, N, method, d_W, d_nnd, d_nn, d_live, d_flag, d_st);
                hipLaunchKernelGGL(k_linkage_rescan, dim3(groups), dim3(LINK_SCAN_THREADS), 0, nullptr, N, d_W, d_live, d_nnd, d_nn, d_flag, d_st, d_rescanned);
            }
            ONESHOT_CHK(hipGetLastError());
            ONESHOT_CHK(hipMemcpy(&st, d_st, sizeof st, hipMemcpyDeviceToHost));   // the chunk's one synchronisation
        }
        ONESHOT_CHK(hipEventRecord(ev[3], nullptr));
        ONESHOT_CHK(hipEventSynchronize(ev[3]));
        if (st.finished == 2 || st.merges > N - 1) return fail(nullptr, HULK_ERR_HIP, "hulk_linkage: a cached neighbour outside the set (corrupt device memory)");
        merges = st.merges;
        if (merges) {
            ONESHOT_CHK(hipMemcpy(merge_a, d_ma, (size_t)merges * 4, hipMemcpyDeviceToHost));
            ONESHOT_CHK(hipMemcpy(merge_b, d_mb, (size_t)merges * 4, hipMemcpyDeviceToHost));
            ONESHOT_CHK(hipMemcpy(merge_distance, d_md, (size_t)merges * 8, hipMemcpyDeviceToHost));
            ONESHOT_CHK(hipMemcpy(merge_size, d_ms, (size_t)merges * 4, hipMemcpyDeviceToHost));
        }
        std::vector<uint32_t> per_group(groups);
        ONESHOT_CHK(hipMemcpy(per_group.data(), d_rescanned, (size_t)groups * 4, hipMemcpyDeviceToHost));
        for (uint32_t x : per_group) rescans += x;
        float a = 0, b = 0;
        ONESHOT_CHK(hipEventElapsedTime(&a, ev[0], ev[1]));
        ONESHOT_CHK(hipEventElapsedTime(&b, ev[2], ev[3]));
        ms_matrix = a; ms_merge = b;
    }
    *n_merges = merges;
    if (stats) {
        stats->seconds_total = now_s() - t0; stats->kernel_ms_matrix = ms_matrix; stats->kernel_ms_merge = ms_merge;
        stats->merges = merges; stats->components = N - merges; stats->rows_rescanned = rescans;
    }
    return HULK_OK;
}
