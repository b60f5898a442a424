// hulk_links.hip — the links of a sketch collection as a sparse graph (hulk_links): row i lists every j != i with d(i, j) <= tau in
// ascending j, d = entry [i][j] of hulk_smash's matrix (sketch i the subject) bit for bit: hulk_cluster's link rule for one direction,
// the pairs kept instead of counted.  CSR on the host (row_start uint64, col uint32, distance double); no N x N array anywhere.
//   the set           prepared once and resident exactly as in hulk_cluster (hulk_cluster.hip: the same buffers, the same peak of
//                     32 * S * N bytes)
// Per band of band_rows subject rows, with NT = NP / 64 column tiles:
//   k_links_count     the pair tile (SET::tile, called the way k_cluster_link calls it) and an epilogue: the 16
//                     compares of a thread as in k_cluster_link, then the four nibbles of a row's 16 neighbouring lanes combined
//                     into the row's 64-bit mask by shuffles inside those lanes (no LDS, no atomics), one plain 8-byte store per
//                     (row, tile), zeros included: mask[tile][row of the band] — the 32 rows of a workgroup are 256 contiguous bytes.
//                     HULK_LINKS_UPPER: the tiles in front of the band's first row are not launched and never read, those below
//                     the diagonal inside the launched range store their zeros and leave
//   k_links_rows      64 rows x 16 segments of the tile range a workgroup: popcounts per segment, an exclusive scan over the 16
//                     segments through LDS, then offset[tile][row] (uint32) = the edges of the row in front of the tile, and the row's
//                     degree.  A wave is 64 rows of one segment: two ballots a tile say which of the two 32 x 64 tiles hold an
//                     edge, and lane 0 appends those to the tile list (one atomic add on the list's length per tile that holds
//                     an edge; the ORDER of the list is free — it decides which workgroup fills a tile, not where an edge goes)
//   k_links_scan      one workgroup: the exclusive scan of the degrees over the band's rows (64-bit), the band's total, the largest
//                     degree.  The host reads total, list length and largest degree here: ONE synchronisation per band, which also
//                     decides the cap (max_edges) and sizes the band's edge buffer
//   k_links_fill      over the tile list only: the tile again — the same text, so the same bits — and an edge (s, q, d) of a set
//                     mask bit goes to links_slot(row_start[s], offset[tile][s], mask, bit) (hulk_links_place.h): every slot of the
//                     band is written exactly once, by plain stores, whatever the order of the workgroups
//   the copy          col / distance of the band and its row starts go into the host result behind the fill, serially: the next
//                     band's count pass does not run beside them (not measured either way; tools/links_cost.py times the whole call)
// Cost: in the sparse regime this exists for, the second pass touches a handful of tiles.  When everything links it is a second
// full pass: the call costs two passes of the tile plus 12 bytes an edge over the link.
// Device memory beside the set: 12.25 bytes per (row of the band, column tile) — mask 8, offset 4, a list entry per 32 rows — plus
// 12 bytes per edge of the densest band.  The band is shrunk (in steps of 32 rows) until its tables fit in half of the free memory.
// Determinism: a mask bit is a function of the pair; the offsets are functions of the masks; the slot is a function of both.
// Bands, tile shape, list order and scheduling cannot move an edge.
#include "hulk_oneshot.h"

#include <algorithm>
#include <cmath>
#include <new>

#define HULK_LP_FN __host__ __device__ __forceinline__
#include "hulk_links_place.h"

struct hulk_link_list {
    uint32_t n = 0;
    std::vector<uint64_t> row_start;                                // [n + 1]
    std::vector<uint32_t> col;                                      // [edges]
    std::vector<double> dist;                                       // [edges]
};

namespace hulk {
namespace {

constexpr uint32_t LINKS_DEFAULT_BAND = 2048;                       // hulk_cluster's
constexpr uint32_t LINKS_MAX_BAND = 1u << 20;
constexpr uint32_t LINKS_MAX_N = HULK_CLUSTER_MAX_N;
constexpr int LINKS_SEGS = 16, LINKS_SCAN_THREADS = 1024;

struct LinksHead { unsigned long long total; uint32_t tiles, max_degree; };

// subjects b0 + 32 * blockIdx.y .., column tile qt0 + blockIdx.x; mask[tile * band + row of the band]
// links_count is the kernel's text, a function under k_links_count: as the kernel's own body hipcc compiles it to other code (k_dendro_offer, hulk_dendrogram.hip)
template <class SET>
__device__ __forceinline__ void links_count(const SET set, uint32_t N, uint32_t b0, uint32_t qt0, uint32_t S, double tau, uint32_t upper,
                                            uint32_t band, unsigned long long *mask_out) {
    const uint32_t t = qt0 + blockIdx.x, s0 = b0 + blockIdx.y * PAIR_TS, q0 = t * PAIR_TQ;
    unsigned long long *out = mask_out + (size_t)t * band + blockIdx.y * PAIR_TS;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;     // other quad, subject quad inside the tile
    if (upper && s0 >= q0 + PAIR_TQ - 1) {                          // every pair of the tile has s >= q (the whole workgroup leaves)
        if (tid < PAIR_TS) out[tid] = 0;
        return;
    }
    double acc[4][4], uni[4];
    uint32_t cnt[4][4];
    set.tile(s0, set, q0, S, acc, uni, cnt);
    uint32_t mask = 0;                                              // bit 4 * i + j, as in k_cluster_link
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t s = s0 + 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t q = q0 + 4 * tx + j;
            const double d = pair_distance<SET::METRIC>(acc[i][j], uni[i], cnt[i][j], S);
            const bool pair = upper ? s < q : s != q;
            if (s < N && q < N && pair && d <= tau) mask |= 1u << (4 * i + j);         // (a NaN compares false)
        }
    }
    // a row's 64 others sit in the 16 lanes of this ty.  Inside a quad of lanes, lane k takes row k: the nibbles of row k of the
    // quad's four lanes; then the four quads' 16-bit pieces are OR-ed across the 16 lanes.  Every lane of the wave is here
    const int lane = tid & 63, k = tx & 3, quad = lane & ~3;
    uint32_t piece = 0;
#pragma unroll
    for (int l = 0; l < 4; l++) piece |= (((uint32_t)__shfl((int)mask, quad + l) >> (4 * k)) & 15u) << (4 * l);
    unsigned long long word = (unsigned long long)piece << (16 * (tx >> 2));
    word |= __shfl_xor(word, 4);
    word |= __shfl_xor(word, 8);
    if (tx < 4) out[4 * ty + tx] = word;                            // lane k of the first quad: row 4 * ty + k
}

// (mT, wT, NP and not the set: k_dendro_offer, hulk_dendrogram.hip)
template <class SET>
__global__ __launch_bounds__(128) void k_links_count(const double *__restrict__ mT, const double *__restrict__ wT, uint32_t NP, uint32_t N,
                                                     uint32_t b0, uint32_t qt0, uint32_t S, double tau, uint32_t upper,
                                                     uint32_t band, unsigned long long *mask_out) {
    links_count(SET::view(mT, wT, NP, S), N, b0, qt0, S, tau, upper, band, mask_out);
}

// rows32: the band's rows rounded up to 32 (the rows k_links_count stored masks for); tiles qt0 .. NT - 1.
// blockDim (64, LINKS_SEGS): thread (x, y) row 64 * blockIdx.x + x, segment y of the tile range
__global__ __launch_bounds__(64 * LINKS_SEGS) void k_links_rows(const unsigned long long *__restrict__ mask, uint32_t band, uint32_t rows32, uint32_t qt0,
                                                               uint32_t NT, uint32_t *__restrict__ offset, uint32_t *__restrict__ degree,
                                                               unsigned long long *__restrict__ list, LinksHead *head) {
    __shared__ uint32_t seg_count[LINKS_SEGS][64];
    const uint32_t x = threadIdx.x, y = threadIdx.y, r = blockIdx.x * 64 + x;
    const bool live = r < rows32;
    const uint32_t per = (NT - qt0 + LINKS_SEGS - 1) / LINKS_SEGS;
    const uint32_t ta = qt0 + y * per < NT ? qt0 + y * per : NT, tb = ta + per < NT ? ta + per : NT;
    uint32_t running = 0;
    if (live) for (uint32_t t = ta; t < tb; t++) links_advance(mask[(size_t)t * band + r], &running);
    seg_count[y][x] = running;
    __syncthreads();
    uint32_t front = 0, all = 0;
    for (uint32_t z = 0; z < (uint32_t)LINKS_SEGS; z++) { const uint32_t c = seg_count[z][x]; front += z < y ? c : 0u; all += c; }
    if (live && y == 0) degree[r] = all;
    running = front;
    for (uint32_t t = ta; t < tb; t++) {                            // (the whole wave: one y, the same ta and tb)
        const unsigned long long m = live ? mask[(size_t)t * band + r] : 0ull;
        if (live) offset[(size_t)t * band + r] = links_advance(m, &running);
        const unsigned long long any = __ballot(m != 0);
        if (x == 0) {
            if (any & 0xffffffffull) list[atomicAdd(&head->tiles, 1u)] = (unsigned long long)(2 * blockIdx.x) << 32 | t;
            if (any >> 32) list[atomicAdd(&head->tiles, 1u)] = (unsigned long long)(2 * blockIdx.x + 1) << 32 | t;
        }
    }
}

// one workgroup.  row_start[r] = the edges of the band's rows in front of r; thread i takes the rows i * per .. (i + 1) * per - 1
__global__ __launch_bounds__(LINKS_SCAN_THREADS) void k_links_scan(const uint32_t *__restrict__ degree, uint32_t rows, unsigned long long *__restrict__ row_start,
                                                                  LinksHead *head) {
    __shared__ unsigned long long part[LINKS_SCAN_THREADS];
    __shared__ uint32_t big[LINKS_SCAN_THREADS];
    const uint32_t i = threadIdx.x, per = (rows + LINKS_SCAN_THREADS - 1) / LINKS_SCAN_THREADS;
    const uint32_t ra = i * per < rows ? i * per : rows, rb = ra + per < rows ? ra + per : rows;
    unsigned long long sum = 0; uint32_t mx = 0;
    for (uint32_t r = ra; r < rb; r++) { const uint32_t d = degree[r]; sum += d; mx = d > mx ? d : mx; }
    part[i] = sum; big[i] = mx;
    __syncthreads();
    if (i == 0) {
        unsigned long long at = 0; uint32_t m = 0;
        for (int z = 0; z < LINKS_SCAN_THREADS; z++) { const unsigned long long c = part[z]; part[z] = at; at += c; m = big[z] > m ? big[z] : m; }
        head->total = at; head->max_degree = m;
    }
    __syncthreads();
    unsigned long long at = part[i];
    for (uint32_t r = ra; r < rb; r++) { row_start[r] = at; at += degree[r]; }
}

// workgroup e fills the tile list[e] = (32-row block of the band) << 32 | column tile
// (links_fill: a function under its kernel as links_count is)
template <class SET>
__device__ __forceinline__ void links_fill(const SET set, uint32_t b0, uint32_t S, uint32_t band, const unsigned long long *__restrict__ list,
                                           const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ offset,
                                           const unsigned long long *__restrict__ row_start, uint32_t *__restrict__ col, double *__restrict__ dist) {
    const unsigned long long entry = list[blockIdx.x];
    const uint32_t by = (uint32_t)(entry >> 32), t = (uint32_t)entry, s0 = b0 + by * PAIR_TS, q0 = t * PAIR_TQ;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4], uni[4];
    uint32_t cnt[4][4];
    set.tile(s0, set, q0, S, acc, uni, cnt);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t r = by * PAIR_TS + 4 * ty + i;
        const unsigned long long m = mask[(size_t)t * band + r];
        if (!links_quad_of(m, tx)) continue;
        const unsigned long long start = row_start[r];
        const uint32_t off = offset[(size_t)t * band + r];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t bit = 4 * tx + j;
            if (!((m >> bit) & 1ull)) continue;
            const unsigned long long slot = links_slot(start, off, m, bit);
            col[slot] = q0 + bit;
            dist[slot] = pair_distance<SET::METRIC>(acc[i][j], uni[i], cnt[i][j], S);
        }
    }
}

template <class SET>
__global__ __launch_bounds__(128) void k_links_fill(const double *__restrict__ mT, const double *__restrict__ wT, uint32_t NP, uint32_t b0,
                                                    uint32_t S, uint32_t band, const unsigned long long *__restrict__ list,
                                                    const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ offset,
                                                    const unsigned long long *__restrict__ row_start, uint32_t *__restrict__ col, double *__restrict__ dist) {
    links_fill(SET::view(mT, wT, NP, S), b0, S, band, list, mask, offset, row_start, col, dist);
}

}  // namespace
}  // namespace hulk

using namespace hulk;

extern "C" int hulk_links(int device, const uint64_t *mins, const double *weights, uint32_t n, uint32_t sketch_size,
                          const hulk_links_opts *opts, hulk_link_list **out, hulk_links_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (out) *out = nullptr;
    if (const int rc = collection_args("hulk_links", mins, weights, opts, out != nullptr, n, sketch_size, LINKS_MAX_N)) return rc;
    if (!(opts->max_distance >= 0.0 && opts->max_distance <= 1.0)) return fail(nullptr, HULK_ERR_ARG, "hulk_links: max_distance must be in [0, 1]");
    if (opts->band_rows % 32) return fail(nullptr, HULK_ERR_ARG, "hulk_links: band_rows must be a multiple of 32");
    if (const int rc = collection_flags("hulk_links", opts, HULK_LINKS_UPPER)) return rc;
    const double t0 = now_s();
    if (const int rc = oneshot_device(device)) return rc;
    const uint32_t N = n, S = sketch_size, NP = smash_padded_n(N), NT = NP / PAIR_TQ;
    const int metric = opts->metric;
    const double tau = opts->max_distance;
    const uint32_t upper = (opts->flags & HULK_LINKS_UPPER) ? 1u : 0u;
    const uint64_t cap = opts->max_edges;
    OneShot own;
    double *d_mT = nullptr, *d_wT = nullptr;
    if (const int rc = prepare_set(own, metric, mins, weights, N, S, d_mT, d_wT)) return rc;      // (the peak: hulk_cluster.hip's header comment)
    // the band: the caller's, capped as in hulk_cluster, no longer than the set, and short enough for its tables (the header comment)
    uint32_t band = opts->band_rows ? std::min(opts->band_rows, LINKS_MAX_BAND) : LINKS_DEFAULT_BAND;
    band = std::min(band, (N + 31) / 32 * 32);
    {
        size_t free_b = 0, total_b = 0;
        ONESHOT_CHK(hipMemGetInfo(&free_b, &total_b));
        const size_t per_row = (size_t)NT * 12 + (size_t)NT / 4 + 16;
        const size_t fit = (free_b / 2) / per_row / 32 * 32;
        if (fit < band) band = (uint32_t)std::max<size_t>(fit, 32);
    }
    const size_t cells = (size_t)band * NT;
    unsigned long long *d_mask = nullptr, *d_list = nullptr, *d_row_start = nullptr;
    uint32_t *d_offset = nullptr, *d_degree = nullptr, *d_col = nullptr; double *d_dist = nullptr;
    LinksHead *d_head = nullptr;
    ONESHOT_CHK(own.alloc(&d_mask, cells)); ONESHOT_CHK(own.alloc(&d_offset, cells));
    ONESHOT_CHK(own.alloc(&d_list, (size_t)(band / 32) * NT));
    ONESHOT_CHK(own.alloc(&d_degree, band)); ONESHOT_CHK(own.alloc(&d_row_start, band)); ONESHOT_CHK(own.alloc(&d_head, 1));
    size_t edge_cap = 0;                                            // of d_col / d_dist: they grow to the densest band
    hipEvent_t ev[4];
    for (hipEvent_t &e : ev) ONESHOT_CHK(own.event(&e));
    hulk_link_list *list = new (std::nothrow) hulk_link_list;
    if (!list) return fail(nullptr, HULK_ERR_HIP, "hulk_links: out of host memory");
    struct Guard { hulk_link_list *l; ~Guard() { delete l; } } guard{list};
    uint64_t edges = 0;
    uint32_t bands = 0, max_degree = 0;
    double ms_count = 0.0, ms_fill = 0.0;
    try {
        list->n = N;
        list->row_start.assign((size_t)N + 1, 0);
        for (uint64_t b0 = 0; b0 < N; b0 += band, bands++) {
            const uint32_t rows = (uint32_t)std::min<uint64_t>(band, N - b0), rows32 = (rows + 31) / 32 * 32;
            const uint32_t qt0 = upper ? (uint32_t)b0 / PAIR_TQ : 0u;   // upper: the tiles in front of the band's first row lie below the diagonal
            const dim3 g(NT - qt0, rows32 / PAIR_TS);
            ONESHOT_CHK(hipMemsetAsync(d_head, 0, sizeof(LinksHead), nullptr));
            ONESHOT_CHK(hipEventRecord(ev[0], nullptr));
            with_set(metric, d_mT, d_wT, NP, S, [&](auto set) {
                hipLaunchKernelGGL(k_links_count<decltype(set)>, g, dim3(128), 0, nullptr, d_mT, d_wT, NP, N, (uint32_t)b0, qt0, S, tau, upper, band, d_mask);
            });
            ONESHOT_CHK(hipGetLastError());
            ONESHOT_CHK(hipEventRecord(ev[1], nullptr));
            hipLaunchKernelGGL(k_links_rows, dim3((rows32 + 63) / 64), dim3(64, LINKS_SEGS), 0, nullptr, d_mask, band, rows32, qt0, NT, d_offset, d_degree, d_list, d_head);
            ONESHOT_CHK(hipGetLastError());
            hipLaunchKernelGGL(k_links_scan, dim3(1), dim3(LINKS_SCAN_THREADS), 0, nullptr, d_degree, rows, d_row_start, d_head);
            ONESHOT_CHK(hipGetLastError());
            LinksHead head;
            ONESHOT_CHK(hipMemcpy(&head, d_head, sizeof head, hipMemcpyDeviceToHost));     // the band's one synchronisation
            { float x = 0; ONESHOT_CHK(hipEventElapsedTime(&x, ev[0], ev[1])); ms_count += x; }
            edges += head.total;
            max_degree = std::max(max_degree, head.max_degree);
            if (stats) { stats->edges = edges; stats->bands = bands + 1; stats->max_degree = max_degree; }
            if (cap && edges > cap)
                return fail(nullptr, HULK_ERR_ARG, "hulk_links: more than max_edges = " + std::to_string(cap) + " edges: " + std::to_string(edges) +
                                                   " behind row " + std::to_string(b0 + rows - 1));
            if (head.total) {
                if (head.total > edge_cap) {
                    if (d_col) { ONESHOT_CHK(own.release(d_col)); ONESHOT_CHK(own.release(d_dist)); }
                    edge_cap = 0;
                    if (own.alloc(&d_col, head.total) != hipSuccess || own.alloc(&d_dist, head.total) != hipSuccess) {
                        (void)hipGetLastError();
                        return fail(nullptr, HULK_ERR_HIP, "hulk_links: the " + std::to_string(head.total) + " edges of the band from row " + std::to_string(b0) +
                                                           " do not fit in device memory (" + std::to_string(edges) + " edges so far; a smaller band_rows or max_distance)");
                    }
                    edge_cap = head.total;
                }
                ONESHOT_CHK(hipEventRecord(ev[2], nullptr));
                const dim3 fg(head.tiles);
                with_set(metric, d_mT, d_wT, NP, S, [&](auto set) {
                    hipLaunchKernelGGL(k_links_fill<decltype(set)>, fg, dim3(128), 0, nullptr, d_mT, d_wT, NP, (uint32_t)b0, S, band, d_list, d_mask, d_offset, d_row_start, d_col, d_dist);
                });
                ONESHOT_CHK(hipGetLastError());
                ONESHOT_CHK(hipEventRecord(ev[3], nullptr));
                const size_t at = list->col.size();
                list->col.resize(at + head.total); list->dist.resize(at + head.total);
                ONESHOT_CHK(hipMemcpy(list->col.data() + at, d_col, head.total * 4, hipMemcpyDeviceToHost));
                ONESHOT_CHK(hipMemcpy(list->dist.data() + at, d_dist, head.total * 8, hipMemcpyDeviceToHost));
                { float x = 0; ONESHOT_CHK(hipEventElapsedTime(&x, ev[2], ev[3])); ms_fill += x; }
            }
            // the band's row starts count from the band's first edge
            ONESHOT_CHK(hipMemcpy(list->row_start.data() + b0, d_row_start, (size_t)rows * 8, hipMemcpyDeviceToHost));
            const uint64_t base = edges - head.total;
            for (uint32_t r = 0; r < rows; r++) list->row_start[b0 + r] += base;
        }
        list->row_start[N] = edges;
    } catch (const std::bad_alloc &) {
        return fail(nullptr, HULK_ERR_HIP, "hulk_links: out of host memory behind " + std::to_string(edges) + " edges");
    }
    if (stats) {
        stats->seconds_total = now_s() - t0; stats->kernel_ms_count = ms_count; stats->kernel_ms_fill = ms_fill;
        stats->edges = edges; stats->bands = bands; stats->max_degree = max_degree;
    }
    guard.l = nullptr;
    *out = list;
    return HULK_OK;
}

extern "C" int hulk_link_list_info(const hulk_link_list *list, uint32_t *n, uint64_t *edges) {
    if (!list) return HULK_ERR_ARG;
    if (n) *n = list->n;
    if (edges) *edges = list->col.size();
    return HULK_OK;
}
extern "C" const uint64_t *hulk_link_list_row_start(const hulk_link_list *list) { return list ? list->row_start.data() : nullptr; }
extern "C" const uint32_t *hulk_link_list_cols(const hulk_link_list *list) { return list ? list->col.data() : nullptr; }
extern "C" const double *hulk_link_list_distances(const hulk_link_list *list) { return list ? list->dist.data() : nullptr; }
extern "C" void hulk_link_list_free(hulk_link_list *list) { delete list; }
