// hulk_cluster.hip — single-linkage clustering of a sketch collection at a distance threshold (hulk_cluster): sketches i != j are
// linked when d(i, j) <= tau or d(j, i) <= tau, d = HULKdata.GetDistance exactly as k_smash (hulk_pairwise.hip) computes it with i the
// subject; a cluster is a connected component of that graph, label[i] its smallest member.  No N x N array anywhere.
//   the set           prepared once with k_smash_prep, slot-major doubles mT / wT [slot][NP] ((double)min and |w|, zero rows behind N;
//                     NP = N rounded up to 64), resident for the call: 16 * S bytes a sketch.  The raw upload (another 16 * S bytes
//                     a sketch) is freed behind the preparation, so the PEAK of device memory is 32 * S * N bytes (+ 4 * N for the
//                     parents).  The limit on N is the smaller of the device's memory over 32 * S and 2,097,088 sketches (the
//                     set is prepared in one launch whose grid.y is NP / 32; more is HULK_ERR_ARG)
//   parent[N]         uint32, the identity at the start; the union-find of hulk_unionfind.h (hooks the larger root under the
//                     smaller by compare-and-swap: the root of a component is its smallest member whatever the order of the unions)
//   k_cluster_link    the pair tile of hulk_pairtile.h (k_search_dist's, and the loop k_smash has a copy of: 128 threads, 32 subjects x 64 others,
//                     chunks of 32 slots double-buffered through LDS, 16 accumulators adding in slot order) over ONE set, once per
//                     band of band_rows subject rows; the epilogue forms d with the tile's pair_distance, counts the pairs s != q
//                     with d <= tau (per wave, then one 64-bit atomic per workgroup) and unites them.  Resources and what the
//                     shared tile was measured to cost against a loop of the kernel's own: DESIGN 4d
//                     jaccard: d(s, q) and d(q, s) are the same bits — tiles wholly below the diagonal are not launched or leave
//                     at once, inside the others only s < q is taken and counts twice.  weighted jaccard: the full square, every
//                     ordered pair once, as subject.  One template over the set type (PairSet<0>, PairSet<1>, BottomkSet: symmetric,
//                     taken as jaccard is)
//   k_cluster_flatten parent[i] = root(i), once behind the last band: its output is `label`.  (Behind EVERY band it would keep the next
//                     band's finds one step deep and show the filter whole components; measured, the link kernel is no faster
//                     for it — path halving and hooking under the smaller root keep the trees shallow — and it costs a launch a
//                     band: DESIGN 4e.  The profiling build runs it so with HULK_CLUSTER_BAND_FLATTEN)
// Visibility: the per-XCD L2s are not coherent, and nothing here needs them to be.  The hooks are agent-scope compare-and-swaps and act
// on memory; a find reads with relaxed agent-scope loads, and a value it reads late is an ancestor still (hulk_unionfind.h); the
// filter's plain loads may be stale too: parent[s] == parent[q] with either value old still says that both have that common ancestor.
// What the labels need to be exact is the kernel boundary between the last k_cluster_link and the last k_cluster_flatten.
#include "hulk_oneshot.h"

#include <algorithm>
#include <cmath>

#define HULK_UF_FN __device__ __forceinline__
#define HULK_UF_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define HULK_UF_CAS(p, e, d) atomicCAS((p), (e), (d))
#include "hulk_unionfind.h"

namespace hulk {
namespace {

constexpr uint32_t CLUSTER_DEFAULT_BAND = 2048;                     // hulk_search's query block
constexpr uint32_t CLUSTER_MAX_BAND = 1u << 20;                     // (band_rows / 32 is grid.y of k_cluster_link)
constexpr uint32_t CLUSTER_MAX_N = HULK_CLUSTER_MAX_N;              // N rounded up to 64, over 32, is grid.y of k_smash_prep (at most 65,535)
static_assert(CLUSTER_MAX_N % 64 == 0 && CLUSTER_MAX_N / 32 <= 65535, "k_smash_prep's grid");

// set: the prepared set (NP rows).  Subjects b0 + 32 * blockIdx.y .. (below N), others 64 * (qt0 + blockIdx.x) .. (below N).
// filter: skip a pair whose two parents are equal already (plain loads; it pays where links are dense: DESIGN 4e).
// links: the ordered pairs s != q with d(s, q) <= tau.  METRIC 0 (jaccard, bottomk) is symmetric: the triangle, a link counts twice
// cluster_link is the kernel's text, a function under k_cluster_link: as the kernel's own body hipcc compiles it to other code (k_dendro_offer, hulk_dendrogram.hip)
template <class SET>
__device__ __forceinline__ void cluster_link(const SET set, uint32_t N, uint32_t b0, uint32_t qt0, uint32_t S, double tau, uint32_t filter,
                                             uint32_t *parent, unsigned long long *links, uint32_t *err) {
    const uint32_t s0 = b0 + blockIdx.y * PAIR_TS, q0 = (qt0 + blockIdx.x) * PAIR_TQ;
    if (SET::METRIC == 0 && s0 >= q0 + PAIR_TQ - 1) return;         // jaccard: every pair of the tile has s >= q (the whole workgroup leaves)
    __shared__ uint32_t wg_links;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;     // other quad, subject quad inside the tile
    if (tid == 0) wg_links = 0;                                     // (ordered before its use by the tile's barriers)
    double acc[4][4], uni[4];
    uint32_t cnt[4][4];
    set.tile(s0, set, q0, S, acc, uni, cnt);
    // the epilogue.  First the 16 compares into one word — the accumulators are dead behind it, the unions run on a handful of registers
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t s = s0 + 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t q = q0 + 4 * tx + j;
            const double d = pair_distance<SET::METRIC>(acc[i][j], uni[i], cnt[i][j], S);
            const bool pair = SET::METRIC == 1 ? s != q : s < q;    // (jaccard: (q, s) is this pair again, bit for bit)
            if (s < N && q < N && pair && d <= tau) mask |= 1u << (4 * i + j);         // (a NaN compares false)
        }
    }
    uint32_t mine = (uint32_t)__popc(mask) * (SET::METRIC == 1 ? 1u : 2u);
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

// (mT, wT, NP and not the set: k_dendro_offer, hulk_dendrogram.hip)
template <class SET>
__global__ __launch_bounds__(128) void k_cluster_link(const double *__restrict__ mT, const double *__restrict__ wT, uint32_t NP, uint32_t N,
                                                      uint32_t b0, uint32_t qt0, uint32_t S, double tau, uint32_t filter,
                                                      uint32_t *parent, unsigned long long *links, uint32_t *err) {
    cluster_link(SET::view(mT, wT, NP, S), N, b0, qt0, S, tau, filter, parent, links, err);
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

}  // namespace
}  // namespace hulk

using namespace hulk;

extern "C" int hulk_cluster(int device, const uint64_t *mins, const double *weights, uint32_t n, uint32_t sketch_size,
                            const hulk_cluster_opts *opts, uint32_t *label, hulk_cluster_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (const int rc = collection_args("hulk_cluster", mins, weights, opts, label != nullptr, n, sketch_size, CLUSTER_MAX_N)) return rc;
    if (!(opts->max_distance >= 0.0 && opts->max_distance <= 1.0)) return fail(nullptr, HULK_ERR_ARG, "hulk_cluster: max_distance must be in [0, 1]");
    if (opts->band_rows % 32) return fail(nullptr, HULK_ERR_ARG, "hulk_cluster: band_rows must be a multiple of 32");
    if (const int rc = collection_flags("hulk_cluster", opts, 0)) return rc;
    const double t0 = now_s();
    if (const int rc = oneshot_device(device)) return rc;
    const uint32_t N = n, S = sketch_size, NP = smash_padded_n(N), band = opts->band_rows ? std::min(opts->band_rows, CLUSTER_MAX_BAND) : CLUSTER_DEFAULT_BAND;
    const int metric = opts->metric;
    const double tau = opts->max_distance;
    // experiments (tools/cluster_cost.py, the profiling build only): what the filter and a flatten behind every band are worth
    const uint32_t filter = HULK_EXP_ENV("HULK_CLUSTER_NO_FILTER") ? 0u : 1u;
    const bool band_flatten = HULK_EXP_ENV("HULK_CLUSTER_BAND_FLATTEN") != nullptr;
    OneShot own;                                                    // events per band: before the link kernel, behind it, behind the flatten (if one ran)
    unsigned long long *d_links = nullptr; double *d_mT = nullptr, *d_wT = nullptr;
    uint32_t *d_parent = nullptr, *d_err = nullptr;
    ONESHOT_CHK(own.alloc(&d_parent, N)); ONESHOT_CHK(own.alloc(&d_links, 1)); ONESHOT_CHK(own.alloc(&d_err, 1));
    // (the peak of device memory: the header comment — these three and the set with its staging, whichever is allocated first.
    // bottomk: the same buffers hold the sorted run-length form, BottomkSet::view)
    if (const int rc = prepare_set(own, metric, mins, weights, N, S, d_mT, d_wT)) return rc;
    {   // the identity (label doubles as the host staging)
        for (uint32_t i = 0; i < N; i++) label[i] = i;
        ONESHOT_CHK(hipMemcpy(d_parent, label, (size_t)N * 4, hipMemcpyHostToDevice));
    }
    ONESHOT_CHK(hipMemset(d_links, 0, 8)); ONESHOT_CHK(hipMemset(d_err, 0, 4));
    // the bands are queued back to back and timed by events that are read behind one synchronisation at the end: the device does
    // not wait for the host between them
    uint32_t bands = 0;
    std::vector<uint8_t> flattened;
    const std::vector<hipEvent_t> &ev = own.events;
    auto mark = [&]() -> hipError_t {
        hipEvent_t e = nullptr;
        const hipError_t rc = own.event(&e);
        return rc != hipSuccess ? rc : hipEventRecord(e, nullptr);
    };
    const dim3 fg((N + 255) / 256);
    for (uint64_t b0 = 0; b0 < N; b0 += band, bands++) {
        const uint32_t rows = (uint32_t)std::min<uint64_t>(band, N - b0);
        // jaccard: the tiles in front of the band's first row lie below the diagonal
        const uint32_t qt0 = metric == HULK_METRIC_WEIGHTED_JACCARD ? 0u : (uint32_t)b0 / PAIR_TQ;
        const dim3 g(NP / PAIR_TQ - qt0, (rows + PAIR_TS - 1) / PAIR_TS);
        const bool last = b0 + band >= N;
        ONESHOT_CHK(mark());
        with_set(metric, d_mT, d_wT, NP, S, [&](auto set) {
            hipLaunchKernelGGL(k_cluster_link<decltype(set)>, g, dim3(128), 0, nullptr, d_mT, d_wT, NP, N, (uint32_t)b0, qt0, S, tau, filter, d_parent, d_links, d_err);
        });
        ONESHOT_CHK(hipGetLastError());
        ONESHOT_CHK(mark());
        flattened.push_back(band_flatten || last);
        if (flattened.back()) {
            hipLaunchKernelGGL(k_cluster_flatten, fg, dim3(256), 0, nullptr, d_parent, N, d_err);
            ONESHOT_CHK(hipGetLastError());
        }
        ONESHOT_CHK(mark());
    }
    ONESHOT_CHK(hipEventSynchronize(ev.back()));
    double ms_link = 0.0, ms_flatten = 0.0;
    for (uint32_t b = 0; b < bands; b++) {
        float x = 0, y = 0;
        ONESHOT_CHK(hipEventElapsedTime(&x, ev[3 * b], ev[3 * b + 1]));
        ms_link += x;
        if (flattened[b]) { ONESHOT_CHK(hipEventElapsedTime(&y, ev[3 * b + 1], ev[3 * b + 2])); ms_flatten += y; }
    }
    uint32_t err = 0; unsigned long long links = 0;
    ONESHOT_CHK(hipMemcpy(&err, d_err, 4, hipMemcpyDeviceToHost));
    ONESHOT_CHK(hipMemcpy(&links, d_links, 8, hipMemcpyDeviceToHost));
    ONESHOT_CHK(hipMemcpy(label, d_parent, (size_t)N * 4, hipMemcpyDeviceToHost));
    if (err) return fail(nullptr, HULK_ERR_HIP, "hulk_cluster: a parent larger than its node was read (corrupt device memory)");
    uint32_t clusters = 0;
    for (uint32_t i = 0; i < N; i++) clusters += label[i] == i;
    if (stats) {
        stats->seconds_total = now_s() - t0; stats->kernel_ms_link = ms_link; stats->kernel_ms_flatten = ms_flatten;
        stats->links = links; stats->bands = bands; stats->clusters = clusters;
    }
    return HULK_OK;
}
