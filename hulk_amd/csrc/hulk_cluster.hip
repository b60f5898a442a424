// hulk_cluster.hip — single-linkage clustering of a sketch collection at a distance threshold (hulk_cluster): sketches i != j are
// linked when d(i, j) <= tau or d(j, i) <= tau, d = HULKdata.GetDistance exactly as k_smash (hulk_cws.hip) computes it with i the
// subject; a cluster is a connected component of that graph, label[i] its smallest member.  No N x N array anywhere.
//   the set           prepared once with k_smash_prep, slot-major doubles mT / wT [slot][NP] ((double)min and |w|, zero rows behind N;
//                     NP = N rounded up to 64), resident for the call: 16 * S bytes a sketch.  The raw upload (another 16 * S bytes
//                     a sketch) is freed behind the preparation, so the PEAK of device memory is 32 * S * N bytes (+ 4 * N for the
//                     parents).  The limit on N is the smaller of the device's memory over 32 * S and 2,097,088 sketches (the
//                     set is prepared in one launch whose grid.y is NP / 32; more is HULK_ERR_ARG)
//   parent[N]         uint32, the identity at the start; the union-find of hulk_unionfind.h (hooks the larger root under the
//                     smaller by compare-and-swap: the root of a component is its smallest member whatever the order of the unions)
//   k_cluster_link    k_search_dist's register tile (hulk_search.hip: 128 threads, 32 subjects x 64 others, chunks of 32 slots
//                     double-buffered through LDS, 16 accumulators adding in slot order) over ONE set, once per band of band_rows
//                     subject rows; the epilogue forms d with k_search_dist's expression, counts the pairs s != q with d <= tau
//                     (per wave, then one 64-bit atomic per workgroup) and unites them.  The main loop is a COPY of k_search_dist's:
//                     as a shared device function template it cost k_search_dist two VGPRs, so that kernel stays as it is
//                     jaccard: d(s, q) and d(q, s) are the same bits — tiles wholly below the diagonal are not launched or leave
//                     at once, inside the others only s < q is taken and counts twice.  weighted jaccard: the full square, every
//                     ordered pair once, as subject
//   k_cluster_flatten parent[i] = root(i), once behind the last band: its output is `label`.  (Behind EVERY band it would keep the next
//                     band's finds one step deep and show the filter whole components; measured, the link kernel is no faster
//                     for it — path halving and hooking under the smaller root keep the trees shallow — and it costs a launch a
//                     band: DESIGN 4e.  The profiling build runs it so with HULK_CLUSTER_BAND_FLATTEN)
// Visibility: the per-XCD L2s are not coherent, and nothing here needs them to be.  The hooks are agent-scope compare-and-swaps and act
// on memory; a find reads with relaxed agent-scope loads, and a value it reads late is an ancestor still (hulk_unionfind.h); the
// filter's plain loads may be stale too: parent[s] == parent[q] with either value old still says that both have that common ancestor.
// What the labels need to be exact is the kernel boundary between the last k_cluster_link and the last k_cluster_flatten.
#include "hulk_ctx.h"

#include <algorithm>
#include <chrono>
#include <cmath>

#define HULK_UF_FN __device__ __forceinline__
#define HULK_UF_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define HULK_UF_CAS(p, e, d) atomicCAS((p), (e), (d))
#include "hulk_unionfind.h"

namespace hulk {
namespace {

constexpr int CLUSTER_TS = 32, CLUSTER_TQ = 64, CLUSTER_CH = 32, CLUSTER_PAD = 2;
constexpr uint32_t CLUSTER_DEFAULT_BAND = 2048;                     // hulk_search's query block
constexpr uint32_t CLUSTER_MAX_BAND = 1u << 20;                     // (band_rows / 32 is grid.y of k_cluster_link)
constexpr uint32_t CLUSTER_MAX_N = HULK_CLUSTER_MAX_N;              // N rounded up to 64, over 32, is grid.y of k_smash_prep (at most 65,535)
static_assert(CLUSTER_MAX_N % 64 == 0 && CLUSTER_MAX_N / 32 <= 65535, "k_smash_prep's grid");

// mT / wT: the prepared set [S][NP].  Subjects b0 + 32 * blockIdx.y .. (below N), others 64 * (qt0 + blockIdx.x) .. (below N).
// filter: skip a pair whose two parents are equal already (plain loads; it pays where links are dense: DESIGN 4e).
// links: the ordered pairs s != q with d(s, q) <= tau
template <int METRIC>
__global__ __launch_bounds__(128) void k_cluster_link(const double *__restrict__ mT, const double *__restrict__ wT, uint32_t NP, uint32_t N,
                                                      uint32_t b0, uint32_t qt0, uint32_t S, double tau, uint32_t filter,
                                                      uint32_t *parent, unsigned long long *links, uint32_t *err) {
    const uint32_t s0 = b0 + blockIdx.y * CLUSTER_TS, q0 = (qt0 + blockIdx.x) * CLUSTER_TQ;
    if (METRIC == 0 && s0 >= q0 + CLUSTER_TQ - 1) return;           // jaccard: every pair of the tile has s >= q (the whole workgroup leaves)
    __shared__ __align__(16) double ma[2][CLUSTER_CH][CLUSTER_TS + CLUSTER_PAD], wa[METRIC == 1 ? 2 : 1][METRIC == 1 ? CLUSTER_CH : 1][CLUSTER_TS + CLUSTER_PAD];
    __shared__ __align__(16) double mb[2][CLUSTER_CH][CLUSTER_TQ + CLUSTER_PAD];
    __shared__ uint32_t wg_links;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;     // other quad, subject quad inside the tile
    // staging: thread t moves slot (t / 4) of the chunk: 8 subject rows (mins, weights) and 16 other rows from (t % 4) on
    const int lc = tid >> 2, lr = tid & 3;
    if (tid == 0) wg_links = 0;                                     // (ordered before its use by the loop's barriers)
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
        const bool ok = col < S;
        const double2 *pa = (const double2 *)(mT + (size_t)col * NP + s0 + 8 * lr);
        const double2 *pw = (const double2 *)(wT + (size_t)col * NP + s0 + 8 * lr);
        const double2 *pb = (const double2 *)(mT + (size_t)col * NP + q0 + 16 * lr);
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
    for (uint32_t c0 = 0; c0 < S; c0 += CLUSTER_CH, buf ^= 1) {
        const bool more = c0 + CLUSTER_CH < S;
        if (more) fetch(c0 + CLUSTER_CH);                           // in flight under this chunk's arithmetic
        const uint32_t lim = S - c0 < (uint32_t)CLUSTER_CH ? S - c0 : (uint32_t)CLUSTER_CH;
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
    // the epilogue.  First the 16 compares into one word — the accumulators are dead behind it, the unions run on a handful of registers
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t s = s0 + 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t q = q0 + 4 * tx + j;
            const double d = METRIC == 1 ? 1 - (acc[i][j] / uni[i]) : 1.0 - ((double)cnt[i][j] / (double)S);
            const bool pair = METRIC == 1 ? s != q : s < q;         // (jaccard: (q, s) is this pair again, bit for bit)
            if (s < N && q < N && pair && d <= tau) mask |= 1u << (4 * i + j);         // (a NaN compares false)
        }
    }
    uint32_t mine = (uint32_t)__popc(mask) * (METRIC == 1 ? 1u : 2u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((tid & 63) == 0 && mine) atomicAdd(&wg_links, mine);        // (at most 2 x 2048 a workgroup)
    while (mask) {
        const int bit = __ffs((int)mask) - 1;
        mask &= mask - 1;
        const uint32_t s = s0 + 4 * ty + (uint32_t)(bit >> 2), q = q0 + 4 * tx + (uint32_t)(bit & 3);
        if (filter && parent[s] == parent[q]) continue;             // one component already (plain loads; a stale value is an ancestor too)
        uf_unite(parent, s, q, err);
    }
    __syncthreads();
    if (tid == 0 && wg_links) atomicAdd(links, (unsigned long long)wg_links);
}

// parent[i] = root(i).  No hook runs beside this kernel, so the roots stand still and every store writes the value the node ends with
__global__ __launch_bounds__(256) void k_cluster_flatten(uint32_t *parent, uint32_t N, uint32_t *err) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    uint32_t x = i;
    for (;;) {                                                      // (the variant: x decreases)
        const uint32_t p = HULK_UF_LOAD(&parent[x]);
        if (p == x) break;
        if (p > x) { atomicCAS(err, 0u, 1u); return; }
        x = p;
    }
    __hip_atomic_store(&parent[i], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace
}  // namespace hulk

using namespace hulk;

extern "C" int hulk_cluster(int device, const uint64_t *mins, const double *weights, uint32_t n, uint32_t sketch_size,
                            const hulk_cluster_opts *opts, uint32_t *label, hulk_cluster_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!mins || !weights || !opts || !label) return fail(nullptr, HULK_ERR_ARG, "hulk_cluster: NULL");
    if (n == 0 || sketch_size == 0) return fail(nullptr, HULK_ERR_ARG, "hulk_cluster: n and sketch_size must be positive");
    if (n > CLUSTER_MAX_N) return fail(nullptr, HULK_ERR_ARG, "hulk_cluster: n must be at most " + std::to_string(CLUSTER_MAX_N));
    if (opts->metric != HULK_METRIC_JACCARD && opts->metric != HULK_METRIC_WEIGHTED_JACCARD) return fail(nullptr, HULK_ERR_ARG, "hulk_cluster: metric");
    if (!(opts->max_distance >= 0.0 && opts->max_distance <= 1.0)) return fail(nullptr, HULK_ERR_ARG, "hulk_cluster: max_distance must be in [0, 1]");
    if (opts->band_rows % 32) return fail(nullptr, HULK_ERR_ARG, "hulk_cluster: band_rows must be a multiple of 32");
    if (opts->flags) return fail(nullptr, HULK_ERR_ARG, "hulk_cluster: unknown flags");
    for (uint64_t x : opts->reserved) if (x) return fail(nullptr, HULK_ERR_ARG, "hulk_cluster: reserved fields must be zero");
    const double t0 = now_s();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, HULK_ERR_NO_DEVICE);
    if (device < 0 || device >= ndev) return fail(nullptr, HULK_ERR_ARG, "device ordinal");
    const uint32_t N = n, S = sketch_size, NP = smash_padded_n(N), band = opts->band_rows ? std::min(opts->band_rows, CLUSTER_MAX_BAND) : CLUSTER_DEFAULT_BAND;
    const int metric = opts->metric;
    const double tau = opts->max_distance;
    // experiments (tools/cluster_cost.py, the profiling build only): what the filter and a flatten behind every band are worth
    const uint32_t filter = HULK_EXP_ENV("HULK_CLUSTER_NO_FILTER") ? 0u : 1u;
    const bool band_flatten = HULK_EXP_ENV("HULK_CLUSTER_BAND_FLATTEN") != nullptr;
    const size_t NS = (size_t)N * S, NT = (size_t)NP * S;
    unsigned long long *d_raw_m = nullptr, *d_links = nullptr; double *d_raw_w = nullptr, *d_mT = nullptr, *d_wT = nullptr;
    uint32_t *d_parent = nullptr, *d_err = nullptr;
    std::vector<hipEvent_t> ev;                                     // per band: before the link kernel, behind it, behind the flatten (if one ran)
    auto done = [&](int rc) {
        hipFree(d_raw_m); hipFree(d_raw_w); hipFree(d_mT); hipFree(d_wT); hipFree(d_parent); hipFree(d_links); hipFree(d_err);
        for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
        return rc;
    };
#define CL_CHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return done(fail_hip(nullptr, e_, #call)); } while (0)
    CL_CHK(hipSetDevice(device));
    CL_CHK(hipMalloc((void **)&d_mT, NT * 8)); CL_CHK(hipMalloc((void **)&d_wT, NT * 8));
    CL_CHK(hipMalloc((void **)&d_raw_m, NS * 8)); CL_CHK(hipMalloc((void **)&d_raw_w, NS * 8));
    CL_CHK(hipMalloc((void **)&d_parent, (size_t)N * 4)); CL_CHK(hipMalloc((void **)&d_links, 8)); CL_CHK(hipMalloc((void **)&d_err, 4));
    CL_CHK(hipMemcpy(d_raw_m, mins, NS * 8, hipMemcpyHostToDevice)); CL_CHK(hipMemcpy(d_raw_w, weights, NS * 8, hipMemcpyHostToDevice));
    CL_CHK(launch_panel_prep(nullptr, d_raw_m, d_raw_w, N, S, d_mT, d_wT));
    CL_CHK(hipDeviceSynchronize());
    CL_CHK(hipFree(d_raw_m)); d_raw_m = nullptr;
    CL_CHK(hipFree(d_raw_w)); d_raw_w = nullptr;
    {   // the identity (label doubles as the host staging)
        for (uint32_t i = 0; i < N; i++) label[i] = i;
        CL_CHK(hipMemcpy(d_parent, label, (size_t)N * 4, hipMemcpyHostToDevice));
    }
    CL_CHK(hipMemset(d_links, 0, 8)); CL_CHK(hipMemset(d_err, 0, 4));
    // the bands are queued back to back and timed by events that are read behind one synchronisation at the end: the device does
    // not wait for the host between them
    uint32_t bands = 0;
    std::vector<uint8_t> flattened;
    auto mark = [&]() -> hipError_t {
        hipEvent_t e = nullptr;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        ev.push_back(e);
        return hipEventRecord(e, nullptr);
    };
    const dim3 fg((N + 255) / 256);
    for (uint64_t b0 = 0; b0 < N; b0 += band, bands++) {
        const uint32_t rows = (uint32_t)std::min<uint64_t>(band, N - b0);
        // jaccard: the tiles in front of the band's first row lie below the diagonal
        const uint32_t qt0 = metric == HULK_METRIC_WEIGHTED_JACCARD ? 0u : (uint32_t)b0 / CLUSTER_TQ;
        const dim3 g(NP / CLUSTER_TQ - qt0, (rows + CLUSTER_TS - 1) / CLUSTER_TS);
        const bool last = b0 + band >= N;
        CL_CHK(mark());
        if (metric == HULK_METRIC_WEIGHTED_JACCARD)
            hipLaunchKernelGGL(k_cluster_link<1>, g, dim3(128), 0, nullptr, d_mT, d_wT, NP, N, (uint32_t)b0, qt0, S, tau, filter, d_parent, d_links, d_err);
        else
            hipLaunchKernelGGL(k_cluster_link<0>, g, dim3(128), 0, nullptr, d_mT, d_wT, NP, N, (uint32_t)b0, qt0, S, tau, filter, d_parent, d_links, d_err);
        CL_CHK(hipGetLastError());
        CL_CHK(mark());
        flattened.push_back(band_flatten || last);
        if (flattened.back()) {
            hipLaunchKernelGGL(k_cluster_flatten, fg, dim3(256), 0, nullptr, d_parent, N, d_err);
            CL_CHK(hipGetLastError());
        }
        CL_CHK(mark());
    }
    CL_CHK(hipEventSynchronize(ev.back()));
    double ms_link = 0.0, ms_flatten = 0.0;
    for (uint32_t b = 0; b < bands; b++) {
        float x = 0, y = 0;
        CL_CHK(hipEventElapsedTime(&x, ev[3 * b], ev[3 * b + 1]));
        ms_link += x;
        if (flattened[b]) { CL_CHK(hipEventElapsedTime(&y, ev[3 * b + 1], ev[3 * b + 2])); ms_flatten += y; }
    }
    uint32_t err = 0; unsigned long long links = 0;
    CL_CHK(hipMemcpy(&err, d_err, 4, hipMemcpyDeviceToHost));
    CL_CHK(hipMemcpy(&links, d_links, 8, hipMemcpyDeviceToHost));
    CL_CHK(hipMemcpy(label, d_parent, (size_t)N * 4, hipMemcpyDeviceToHost));
#undef CL_CHK
    if (err) return done(fail(nullptr, HULK_ERR_HIP, "hulk_cluster: a parent larger than its node was read (corrupt device memory)"));
    uint32_t clusters = 0;
    for (uint32_t i = 0; i < N; i++) clusters += label[i] == i;
    if (stats) {
        stats->seconds_total = now_s() - t0; stats->kernel_ms_link = ms_link; stats->kernel_ms_flatten = ms_flatten;
        stats->links = links; stats->bands = bands; stats->clusters = clusters;
    }
    return done(HULK_OK);
}
