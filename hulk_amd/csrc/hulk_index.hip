// hulk_index.hip — a banded index over a sketch collection that stays on the device (hulk_index_build / _search / _save / _load):
// hulk_search's hit lists under positional jaccard at a distance threshold, from the sketches that share a band with the query
// instead of from every sketch.  The rule, the theorem (with bands >= u_max + 1 the result is hulk_search's, bit for bit) and the
// file format stand in include/hulk_hip.h.
//   resident        d_mins [n][S] (double)min, row-major: a wave reads a sketch's row coalesced; d_keys [n][B] the band keys by
//                   sketch; d_skey / d_sidx [B][n] per band the (key, sketch) pairs ascending by (key, sketch): 8 S + 20 B bytes
//                   a sketch
//   k_index_keys    a thread folds one band of one sketch (hash64 over the bits of the doubles, slots ascending); the queries of a
//                   search go through the same kernel
//   k_index_sort_step  the build's sort, per band, a bitonic network in global memory whose compare-exchanges all point upwards
//                   (the first step of a merge mirrors, the others shift), so that n needs no padding: a partner behind n is
//                   +infinity and never moves.  The order (key, sketch) is total: the network's result is the sorted sequence
//   k_index_probe<0>  count: a wave owns (query, band): a binary search for the run of the query's key, then over the run, 64 entries
//                   a step, the sketches for which this band is the FIRST one shared with the query (the by-sketch keys of the
//                   bands before it differ) — every distinct candidate pair is counted in exactly one band
//   k_index_scan    per query the exclusive scan of its B counts and their sum; the host reads the sums in one synchronisation,
//                   cuts the queries into blocks that fit the scratch (a query above it alone goes in pieces) and
//   k_index_probe<1>  fill: the same walk writes every candidate to its final slot: start of the query + offset of the band + rank
//                   in the run (a ballot's population count below the lane).  No atomics, no sort, no dependence on scheduling
//   k_index_verify  a wave owns a candidate: both rows coalesced, the equal slots counted (an integer: any order gives one sum),
//                   1.0 - cnt / S — pair_distance<0>'s expression
//   k_index_select  k_search_select over a candidate list: a wave owns a query, lane l < K entry l of its list under the 96-bit key
//                   (distance bits, index); the list is a function of the set of candidates, whatever order they arrive in
#include "hulk_oneshot.h"
#include "hulk_device.h"
#include "crc32_clmul.h"
#include "hulk_index_plan.h"
#include "hulk_select.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

struct hulk_index {
    int device = 0;
    uint32_t n = 0, S = 0, B = 0;
    double D = 0.0;
    double *d_mins = nullptr;
    unsigned long long *d_keys = nullptr, *d_skey = nullptr;
    uint32_t *d_sidx = nullptr;
    uint64_t device_bytes = 0;
    std::vector<uint64_t> mins;                                     // the raw mins, what hulk_index_save writes
    std::vector<std::string> names;
    // what a search needs beside the index: grown on demand, kept between calls (a service asks one query at a time)
    struct Buf { void *p = nullptr; size_t bytes = 0; } q_raw, q_mins, q_keys, cnt, off, tot, within, seg, cand_p, cand_q, dist, lkey, lidx;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~hulk_index() {
        hipFree(d_mins); hipFree(d_keys); hipFree(d_skey); hipFree(d_sidx);
        for (Buf *b : {&q_raw, &q_mins, &q_keys, &cnt, &off, &tot, &within, &seg, &cand_p, &cand_q, &dist, &lkey, &lidx}) hipFree(b->p);
        for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
    }
};

namespace hulk {
namespace {

constexpr uint64_t INDEX_DEFAULT_SCRATCH = 256ull << 20;
constexpr size_t INDEX_STAGE = 8u << 20;                           // raw mins go up this many entries at a time
constexpr int INDEX_AHEAD = 8;

__global__ __launch_bounds__(256) void k_index_prep(const unsigned long long *__restrict__ raw, size_t count, double *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = (double)raw[i];
}

// keys[i][b], i < n, b < B: band b covers the slots [b S / B, (b + 1) S / B)
__global__ __launch_bounds__(256) void k_index_keys(const double *__restrict__ mins, uint32_t n, uint32_t S, uint32_t B,
                                                    unsigned long long *__restrict__ keys) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n * B) return;
    const uint32_t i = (uint32_t)(t / B), b = (uint32_t)(t % B);
    const uint32_t lo = (uint32_t)((uint64_t)b * S / B), hi = (uint32_t)(((uint64_t)b + 1) * S / B);
    const double *row = mins + (size_t)i * S;
    uint64_t h = 0;
    for (uint32_t s = lo; s < hi; s++) h = hash64(h ^ (uint64_t)__double_as_longlong(row[s]), ~0ull);
    keys[t] = h;
}

__global__ __launch_bounds__(256) void k_index_sort_init(const unsigned long long *__restrict__ keys, uint32_t n, uint32_t B,
                                                         unsigned long long *__restrict__ skey, uint32_t *__restrict__ sidx) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= n) return;
    skey[(size_t)b * n + i] = keys[(size_t)i * B + b];
    sidx[(size_t)b * n + i] = i;
}

// one step of the network over every band (blockIdx.y): thread t owns the pair (i, l), i < l.  mirror: the first step of the merge
// of blocks of 2 j entries, l = i ^ (2 j - 1); otherwise l = i + j.  The larger entry goes to l; l >= n: nothing to do
__global__ __launch_bounds__(256) void k_index_sort_step(unsigned long long *__restrict__ skey, uint32_t *__restrict__ sidx, uint32_t n,
                                                         uint32_t j, uint32_t mirror) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint64_t i64 = (uint64_t)(t / j) * 2 * j + t % j;
    const uint64_t l64 = mirror ? (i64 ^ (2ull * j - 1)) : i64 + j;
    if (l64 >= n) return;
    const size_t base = (size_t)blockIdx.y * n;
    unsigned long long *k = skey + base;
    uint32_t *x = sidx + base;
    const unsigned long long ka = k[i64], kb = k[l64];
    const uint32_t xa = x[i64], xb = x[l64];
    if (ka > kb || (ka == kb && xa > xb)) { k[i64] = kb; k[l64] = ka; x[i64] = xb; x[l64] = xa; }
}

// the walk both probe passes make: a wave owns (query, band) — a thread per pair walked the long runs of a dense collection alone.
// r < mq counts the block's queries, q = qfirst + r is the query's number (under SELF its sketch).  The run of the query's key is
// walked 64 entries a step, lane l the l-th of them; an entry is TAKEN when b is the first band its sketch shares with the query.
// FILL 0: cnt[q][b] = the entries taken.  FILL 1: those sketches to their slots: the candidate's number inside the query is
// off[q][b] + its rank among the taken entries of the run (a ballot's population count below the lane: run order, whatever the
// lanes do); the block holds the numbers [lo, lo + seg_len[r]) at seg_start[r]
template <int FILL>
__global__ __launch_bounds__(256) void k_index_probe(const unsigned long long *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                     const unsigned long long *__restrict__ keys, uint32_t n, uint32_t B,
                                                     const unsigned long long *__restrict__ qkeys, uint32_t qfirst, uint32_t mq, uint32_t self,
                                                     uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                     const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ seg_len, uint32_t lo,
                                                     uint32_t *__restrict__ cand_p, uint32_t *__restrict__ cand_q) {
    const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (w >= (size_t)mq * B) return;                                // (wave-uniform)
    const uint32_t r = (uint32_t)(w / B), b = (uint32_t)(w % B), q = qfirst + r;
    const unsigned long long *qk = qkeys + (size_t)q * B;
    const unsigned long long key = qk[b];
    const unsigned long long *band = skey + (size_t)b * n;
    const uint32_t *who = sidx + (size_t)b * n;
    uint32_t a = 0, z = n;                                          // the first entry of the band that is >= key (the same walk in every lane)
    while (a < z) { const uint32_t mid = a + (z - a) / 2; if (band[mid] < key) a = mid + 1; else z = mid; }
    uint32_t found = 0;
    const uint32_t start = FILL ? seg_start[r] : 0, len = FILL ? seg_len[r] : 0, first = FILL ? off[(size_t)q * B + b] : 0;
    for (uint32_t i0 = a; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool in = i < n && band[i] == key;
        bool take = false;
        uint32_t p = 0;
        if (in) {
            p = who[i];
            take = !(self && p == q);
            const unsigned long long *pk = keys + (size_t)p * B;
            for (uint32_t e = 0; take && e < b; e++) take = pk[e] != qk[e];
        }
        const unsigned long long taken = __ballot(take);
        if (FILL && take) {
            const uint32_t slot = first + found + (uint32_t)__popcll(taken & ((1ull << lane) - 1));
            if (slot >= lo && slot - lo < len) { cand_p[start + (slot - lo)] = p; cand_q[start + (slot - lo)] = q; }
        }
        found += (uint32_t)__popcll(taken);
        if (__ballot(in) != ~0ull) break;                           // the run ends inside these 64 entries
    }
    if (!FILL && lane == 0) cnt[(size_t)q * B + b] = found;
}

// per query of [qfirst, qfirst + mq): off[q][b] = cnt[q][0] + .. + cnt[q][b - 1], tot[q] the sum (a query has at most n candidates)
__global__ __launch_bounds__(256) void k_index_scan(const uint32_t *__restrict__ cnt, uint32_t qfirst, uint32_t mq, uint32_t B,
                                                    uint32_t *__restrict__ off, uint32_t *__restrict__ tot) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= mq) return;
    const size_t at = (size_t)(qfirst + r) * B;
    uint32_t sum = 0;
    for (uint32_t b = 0; b < B; b++) { off[at + b] = sum; sum += cnt[at + b]; }
    tot[qfirst + r] = sum;
}

// a wave owns candidate c < count: dist[c] = 1.0 - equal slots / S of the rows cand_q[c] (queries) and cand_p[c] (the index)
__global__ __launch_bounds__(256) void k_index_verify(const double *__restrict__ qmins, const double *__restrict__ mins, uint32_t S,
                                                      const uint32_t *__restrict__ cand_p, const uint32_t *__restrict__ cand_q, uint32_t count,
                                                      double *__restrict__ dist) {
    const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= count) return;                                         // (wave-uniform)
    const double *a = qmins + (size_t)cand_q[c] * S, *b = mins + (size_t)cand_p[c] * S;
    uint32_t equal = 0;
    for (uint32_t s = lane; s < S; s += 64) equal += a[s] == b[s] ? 1u : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) equal += __shfl_xor(equal, d);
    if (lane == 0) dist[c] = 1.0 - ((double)equal / (double)S);
}

// a wave owns query qfirst + r, r < mq: its candidates are dist / cand_p [seg_start[r], + seg_len[r]).  lkey / lidx [m][K] as in
// k_search_select, kept by the same select_insert (hulk_select.h); within[q] += the candidates with distance <= lim
__global__ __launch_bounds__(256) void k_index_select(const double *__restrict__ dist, const uint32_t *__restrict__ cand_p,
                                                      const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ seg_len,
                                                      uint32_t qfirst, uint32_t mq, uint32_t K, double lim,
                                                      unsigned long long *__restrict__ lkey, uint32_t *__restrict__ lidx,
                                                      uint32_t *__restrict__ within) {
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= mq) return;                                            // (wave-uniform)
    const uint32_t q = qfirst + r, np = seg_len[r];
    const double *row = dist + seg_start[r];
    const uint32_t *who = cand_p + seg_start[r];
    unsigned long long kd = lane < K ? lkey[(size_t)q * K + lane] : ~0ull;
    uint32_t ki = lane < K ? lidx[(size_t)q * K + lane] : ~0u;
    unsigned long long td = __shfl(kd, (int)K - 1);                 // the K-th key: what a candidate has to beat
    uint32_t ti = __shfl(ki, (int)K - 1);
    uint32_t inside = 0;
    for (uint32_t c0 = 0; c0 < np; c0 += 64 * INDEX_AHEAD) {
        double dv[INDEX_AHEAD];
        uint32_t iv[INDEX_AHEAD];
#pragma unroll
        for (int u = 0; u < INDEX_AHEAD; u++) {
            const uint32_t c = c0 + 64 * u + lane;
            dv[u] = c < np ? row[c] : lim;
            iv[u] = c < np ? who[c] : ~0u;
        }
#pragma unroll
        for (int u = 0; u < INDEX_AHEAD; u++) {
            const uint32_t c = c0 + 64 * u + lane, gi = iv[u];
            const double d = dv[u];
            const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
            const bool in = c < np && d >= 0.0 && d <= lim;
            inside += in ? 1u : 0u;
            select_insert(__ballot(in && select_beats(bits, gi, td, ti)), bits, gi, lane, K, kd, ki, td, ti);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) inside += __shfl_xor(inside, d);
    if (lane < K) { lkey[(size_t)q * K + lane] = kd; lidx[(size_t)q * K + lane] = ki; }
    if (lane == 0) within[q] += inside;
}

inline uint32_t blocks_of(size_t threads) { return (uint32_t)((threads + 255) / 256); }
inline uint32_t waves_of(size_t waves) { return (uint32_t)((waves + 3) / 4); }       // workgroups of four waves

// the largest u in [0, S] with 1.0 - (double)(S - u) / (double)S <= D: the distance expression itself
uint32_t index_u_max(uint32_t S, double D) {
    uint32_t u = 0;
    while (u < S && 1.0 - ((double)(S - (u + 1)) / (double)S) <= D) u++;
    return u;
}

template <typename T> hipError_t grow(hulk_index::Buf &b, T **out, size_t count) {
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (b.bytes < bytes) {
        if (b.p) { const hipError_t e = hipFree(b.p); b.p = nullptr; b.bytes = 0; if (e != hipSuccess) return e; }
        const hipError_t e = hipMalloc(&b.p, bytes);
        if (e != hipSuccess) { b.p = nullptr; return e; }
        b.bytes = bytes;
    }
    *out = (T *)b.p;
    return hipSuccess;
}

// rows host sketches [rows][S] (uint64) -> d_out [rows][S] doubles, through the staging buffer d_stage of INDEX_STAGE entries or fewer
hipError_t upload_rows(const uint64_t *mins, size_t count, unsigned long long *d_stage, size_t stage, double *d_out) {
    for (size_t at = 0; at < count; at += stage) {
        const size_t c = std::min(stage, count - at);
        hipError_t e = hipMemcpy(d_stage, mins + at, c * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_index_prep, dim3(blocks_of(c)), dim3(256), 0, nullptr, d_stage, c, d_out + at);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

// what hulk_index_build and hulk_index_load share: the arguments are checked, `mins` is moved into the index
int index_make(int device, std::vector<uint64_t> &&mins, uint32_t n, uint32_t S, double D, uint32_t B, std::vector<std::string> &&names,
               hulk_index **out) {
    if (const int rc = oneshot_device(device)) return rc;
    const uint64_t resident = (uint64_t)n * (8ull * S + 20ull * B);
    const size_t NS = (size_t)n * S, stage = std::min(NS, INDEX_STAGE);
    {
        size_t free_b = 0, total_b = 0;
        ONESHOT_CHK(hipMemGetInfo(&free_b, &total_b));
        const uint64_t need = resident + stage * 8 + (1u << 20);
        if (need > free_b)
            return fail(nullptr, HULK_ERR_HIP, "hulk_index: out of device memory: " + std::to_string(n) + " sketches of " + std::to_string(S) + " slots in " +
                                                   std::to_string(B) + " bands need " + std::to_string(need) + " bytes, " + std::to_string(free_b) + " are free");
    }
    std::unique_ptr<hulk_index> ix(new hulk_index);
    ix->device = device; ix->n = n; ix->S = S; ix->B = B; ix->D = D; ix->device_bytes = resident;
    const size_t NB = (size_t)n * B;
    ONESHOT_CHK(hipMalloc((void **)&ix->d_mins, NS * 8));
    ONESHOT_CHK(hipMalloc((void **)&ix->d_keys, NB * 8));
    ONESHOT_CHK(hipMalloc((void **)&ix->d_skey, NB * 8));
    ONESHOT_CHK(hipMalloc((void **)&ix->d_sidx, NB * 4));
    for (hipEvent_t &e : ix->ev) ONESHOT_CHK(hipEventCreate(&e));
    {
        OneShot own;
        unsigned long long *d_stage = nullptr;
        ONESHOT_CHK(own.alloc(&d_stage, stage));
        ONESHOT_CHK(upload_rows(mins.data(), NS, d_stage, stage, ix->d_mins));
        ONESHOT_CHK(hipDeviceSynchronize());
    }
    hipLaunchKernelGGL(k_index_keys, dim3(blocks_of(NB)), dim3(256), 0, nullptr, ix->d_mins, n, S, B, ix->d_keys);
    ONESHOT_CHK(hipGetLastError());
    ONESHOT_CHK(hipEventRecord(ix->ev[0], nullptr));
    hipLaunchKernelGGL(k_index_sort_init, dim3(blocks_of(n), B), dim3(256), 0, nullptr, ix->d_keys, n, B, ix->d_skey, ix->d_sidx);
    ONESHOT_CHK(hipGetLastError());
    uint64_t P = 1;
    while (P < n) P *= 2;
    const dim3 grid(blocks_of(P / 2), B);
    for (uint64_t k = 2; k <= P; k *= 2) {
        hipLaunchKernelGGL(k_index_sort_step, grid, dim3(256), 0, nullptr, ix->d_skey, ix->d_sidx, n, (uint32_t)(k / 2), 1u);
        for (uint64_t j = k / 4; j >= 1; j /= 2)
            hipLaunchKernelGGL(k_index_sort_step, grid, dim3(256), 0, nullptr, ix->d_skey, ix->d_sidx, n, (uint32_t)j, 0u);
        ONESHOT_CHK(hipGetLastError());
    }
    ONESHOT_CHK(hipEventRecord(ix->ev[1], nullptr));
    ONESHOT_CHK(hipDeviceSynchronize());
    ix->mins = std::move(mins);
    ix->names = std::move(names);
    ix->names.resize(n);
    *out = ix.release();
    return HULK_OK;
}

// a double as %.17g: it reads back to the same value, so two thresholds that differ in the last bit print differently
std::string g17(double v) { char b[40]; snprintf(b, sizeof b, "%.17g", v); return b; }

// the checks of a build's shape, before any HIP call: -> B
int index_shape(const char *who, uint32_t n, uint32_t S, double D, uint32_t bands, uint32_t *B_out) {
    const std::string w = who;
    if (n == 0 || S == 0) return fail(nullptr, HULK_ERR_ARG, w + ": n and sketch_size must be positive");
    if (n == 0xFFFFFFFFu) return fail(nullptr, HULK_ERR_ARG, w + ": too many sketches");
    if (!(D >= 0.0 && D <= 1.0)) return fail(nullptr, HULK_ERR_ARG, w + ": max_distance must be in [0, 1)");
    const uint32_t u_max = index_u_max(S, D);
    if (u_max >= S) return fail(nullptr, HULK_ERR_ARG, w + ": every sketch is within this distance: use hulk_search");
    if (bands > S) return fail(nullptr, HULK_ERR_ARG, w + ": bands must be 0 (derived) or 1 .. sketch_size");
    const uint32_t B = bands ? bands : u_max + 1;
    if (B > INDEX_MAX_BANDS) return fail(nullptr, HULK_ERR_ARG, w + ": more than " + std::to_string(INDEX_MAX_BANDS) + " bands");
    if (!index_threads_ok(n, B))
        return fail(nullptr, HULK_ERR_ARG, w + ": " + std::to_string(n) + " sketches x " + std::to_string(B) + " bands: sketches x bands must be below 2^32");
    *B_out = B;
    return HULK_OK;
}

constexpr char INDEX_MAGIC[8] = {'H', 'U', 'L', 'K', 'I', 'D', 'X', '\n'};
constexpr uint32_t INDEX_FORMAT = 1;
struct IndexHeader {                                                // little-endian, 48 bytes; names (NUL-terminated each), the mins, a CRC-32 follow
    char magic[8];
    uint32_t format, sketch_size, n, bands;
    uint64_t distance_bits, names_bytes, mins_bytes;
};
static_assert(sizeof(IndexHeader) == 48, "the file header is 48 bytes");

}  // namespace
}  // namespace hulk

using namespace hulk;

extern "C" {

int hulk_index_build(int device, const uint64_t *mins, uint32_t n, uint32_t sketch_size, const hulk_index_opts *opts, hulk_index **index) {
    if (index) *index = nullptr;
    if (!mins || !opts || !index) return fail(nullptr, HULK_ERR_ARG, "hulk_index_build: NULL");
    if (opts->metric == HULK_METRIC_WEIGHTED_JACCARD || opts->metric == HULK_METRIC_BOTTOMK)
        return fail(nullptr, HULK_ERR_ARG, "hulk_index_build: only jaccard bounds the number of unequal slots: weightedjaccard and bottomk cannot be indexed");
    if (opts->metric != HULK_METRIC_JACCARD) return fail(nullptr, HULK_ERR_ARG, "hulk_index_build: metric");
    if (opts->flags || opts->pad) return fail(nullptr, HULK_ERR_ARG, "hulk_index_build: unknown flags");
    for (uint64_t x : opts->reserved) if (x) return fail(nullptr, HULK_ERR_ARG, "hulk_index_build: reserved fields must be zero");
    uint32_t B = 0;
    if (const int rc = index_shape("hulk_index_build", n, sketch_size, opts->max_distance, opts->bands, &B)) return rc;
    try {
        std::vector<uint64_t> copy(mins, mins + (size_t)n * sketch_size);      // the handle's host copy: what hulk_index_save writes
        return index_make(device, std::move(copy), n, sketch_size, opts->max_distance, B, {}, index);
    } catch (const std::bad_alloc &) {
        return fail(nullptr, HULK_ERR_HIP, "hulk_index_build: out of host memory: the index keeps a copy of the mins, " +
                                               std::to_string((uint64_t)n * sketch_size * 8) + " bytes");
    }
}

void hulk_index_free(hulk_index *index) {
    if (!index) return;
    hipSetDevice(index->device);
    delete index;
}

int hulk_index_info(const hulk_index *index, uint32_t *n, uint32_t *sketch_size, uint32_t *bands, double *max_distance, uint64_t *device_bytes) {
    if (!index) return fail(nullptr, HULK_ERR_ARG, "hulk_index_info: NULL");
    if (n) *n = index->n;
    if (sketch_size) *sketch_size = index->S;
    if (bands) *bands = index->B;
    if (max_distance) *max_distance = index->D;
    if (device_bytes) *device_bytes = index->device_bytes;
    return HULK_OK;
}

const char *hulk_index_name(const hulk_index *index, uint32_t i) { return (index && i < index->n) ? index->names[i].c_str() : nullptr; }

int hulk_index_set_names(hulk_index *index, const char *const *names, uint32_t n) {
    if (!index || !names) return fail(nullptr, HULK_ERR_ARG, "hulk_index_set_names: NULL");
    if (n != index->n) return fail(nullptr, HULK_ERR_ARG, "hulk_index_set_names: " + std::to_string(n) + " names for " + std::to_string(index->n) + " sketches");
    for (uint32_t i = 0; i < n; i++) if (!names[i]) return fail(nullptr, HULK_ERR_ARG, "hulk_index_set_names: NULL name");
    for (uint32_t i = 0; i < n; i++) index->names[i] = names[i];
    return HULK_OK;
}

static int index_search(hulk_index *index, const uint64_t *q_mins, uint32_t m, const hulk_index_search_opts *opts, uint32_t *hit_index,
                        double *hit_distance, uint32_t *hit_count, hulk_index_search_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!index || !opts || !hit_index || !hit_distance || !hit_count) return fail(nullptr, HULK_ERR_ARG, "hulk_index_search: NULL");
    const uint32_t K = opts->k;
    if (K == 0 || K > HULK_SEARCH_MAX_K) return fail(nullptr, HULK_ERR_ARG, "hulk_index_search: k must be 1 .. " + std::to_string(HULK_SEARCH_MAX_K));
    if (opts->flags & ~HULK_SEARCH_SELF) return fail(nullptr, HULK_ERR_ARG, "hulk_index_search: unknown flags");
    for (uint64_t x : opts->reserved) if (x) return fail(nullptr, HULK_ERR_ARG, "hulk_index_search: reserved fields must be zero");
    const bool self = (opts->flags & HULK_SEARCH_SELF) != 0;
    if (self && q_mins) return fail(nullptr, HULK_ERR_ARG, "hulk_index_search: HULK_SEARCH_SELF takes no queries");
    if (!self && !q_mins) return fail(nullptr, HULK_ERR_ARG, "hulk_index_search: no queries (and no HULK_SEARCH_SELF)");
    if (self) m = index->n;
    if (m == 0) return fail(nullptr, HULK_ERR_ARG, "hulk_index_search: m must be positive");
    double lim = index->D;
    if (opts->max_distance >= 0.0) {
        if (opts->max_distance > index->D)
            return fail(nullptr, HULK_ERR_ARG, "hulk_index_search: max_distance " + g17(opts->max_distance) + " is above the " + g17(index->D) +
                                                   " the index was built for");
        lim = opts->max_distance;
    }
    const uint64_t scratch = opts->scratch_bytes ? opts->scratch_bytes : INDEX_DEFAULT_SCRATCH;
    if (scratch < INDEX_CAND_BYTES)
        return fail(nullptr, HULK_ERR_ARG, "hulk_index_search: scratch_bytes " + std::to_string(scratch) + " is too small for one candidate (" +
                                               std::to_string(INDEX_CAND_BYTES) + " bytes)");
    if (!index_threads_ok(m, index->B))
        return fail(nullptr, HULK_ERR_ARG, "hulk_index_search: " + std::to_string(m) + " queries x " + std::to_string(index->B) +
                                               " bands: queries x bands must be below 2^32");
    const uint32_t cap = index_block_cap(scratch);
    const double t0 = now_s();
    ONESHOT_CHK(hipSetDevice(index->device));
    hulk_index &ix = *index;
    const uint32_t n = ix.n, S = ix.S, B = ix.B;
    const size_t MB = (size_t)m * B, LK = (size_t)m * K;
    const double *d_q = ix.d_mins;
    const unsigned long long *d_qk = ix.d_keys;
    uint32_t *d_cnt = nullptr, *d_off = nullptr, *d_tot = nullptr, *d_within = nullptr, *d_seg = nullptr, *d_lidx = nullptr;
    unsigned long long *d_lkey = nullptr;
    ONESHOT_CHK(hipEventRecord(ix.ev[0], nullptr));
    if (!self) {
        const size_t MS = (size_t)m * S, stage = std::min(MS, INDEX_STAGE);
        unsigned long long *d_raw = nullptr, *d_keys = nullptr; double *d_mins = nullptr;
        ONESHOT_CHK(grow(ix.q_raw, &d_raw, stage)); ONESHOT_CHK(grow(ix.q_mins, &d_mins, MS)); ONESHOT_CHK(grow(ix.q_keys, &d_keys, MB));
        ONESHOT_CHK(upload_rows(q_mins, MS, d_raw, stage, d_mins));
        hipLaunchKernelGGL(k_index_keys, dim3(blocks_of(MB)), dim3(256), 0, nullptr, d_mins, m, S, B, d_keys);
        ONESHOT_CHK(hipGetLastError());
        d_q = d_mins; d_qk = d_keys;
    }
    ONESHOT_CHK(grow(ix.cnt, &d_cnt, MB)); ONESHOT_CHK(grow(ix.off, &d_off, MB)); ONESHOT_CHK(grow(ix.tot, &d_tot, m));
    ONESHOT_CHK(grow(ix.within, &d_within, m)); ONESHOT_CHK(grow(ix.lkey, &d_lkey, LK)); ONESHOT_CHK(grow(ix.lidx, &d_lidx, LK));
    ONESHOT_CHK(hipMemsetAsync(d_within, 0, (size_t)m * 4, nullptr));
    ONESHOT_CHK(hipMemsetAsync(d_lkey, 0xff, LK * 8, nullptr)); ONESHOT_CHK(hipMemsetAsync(d_lidx, 0xff, LK * 4, nullptr));
    ONESHOT_CHK(hipEventRecord(ix.ev[1], nullptr));
    for (uint32_t q0 = 0, chunk = index_count_chunk(B); q0 < m; q0 += std::min(chunk, m - q0)) {      // (a launch stays below 2^32 threads)
        const uint32_t mq = std::min(chunk, m - q0);
        hipLaunchKernelGGL(k_index_probe<0>, dim3(waves_of((size_t)mq * B)), dim3(256), 0, nullptr, ix.d_skey, ix.d_sidx, ix.d_keys, n, B, d_qk, q0,
                           mq, self ? 1u : 0u, d_cnt, (const uint32_t *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr, 0u,
                           (uint32_t *)nullptr, (uint32_t *)nullptr);
        ONESHOT_CHK(hipGetLastError());
        hipLaunchKernelGGL(k_index_scan, dim3(blocks_of(mq)), dim3(256), 0, nullptr, d_cnt, q0, mq, B, d_off, d_tot);
        ONESHOT_CHK(hipGetLastError());
    }
    ONESHOT_CHK(hipEventRecord(ix.ev[2], nullptr));
    std::vector<uint32_t> tot(m);
    ONESHOT_CHK(hipMemcpy(tot.data(), d_tot, (size_t)m * 4, hipMemcpyDeviceToHost));      // the one synchronisation of the count pass
    float f = 0;
    double ms_keys = 0.0, ms_probe = 0.0, ms_verify = 0.0, ms_select = 0.0;
    ONESHOT_CHK(hipEventElapsedTime(&f, ix.ev[0], ix.ev[1])); ms_keys = f;
    ONESHOT_CHK(hipEventElapsedTime(&f, ix.ev[1], ix.ev[2])); ms_probe = f;
    uint64_t candidates = 0;
    for (uint32_t q = 0; q < m; q++) candidates += tot[q];
    const IndexPlan plan = index_plan(tot.data(), m, B, cap);       // (hulk_index_plan.h: every launch below stays under the grid limit)
    const std::vector<IndexBlock> &blocks = plan.blocks;
    const uint32_t n_blocks = plan.query_blocks, n_pieces = plan.pieces, longest = plan.longest;
    const size_t biggest = plan.biggest;
    if (!blocks.empty()) {
        uint32_t *d_cp = nullptr, *d_cq = nullptr; double *d_dist = nullptr;
        ONESHOT_CHK(grow(ix.cand_p, &d_cp, biggest)); ONESHOT_CHK(grow(ix.cand_q, &d_cq, biggest)); ONESHOT_CHK(grow(ix.dist, &d_dist, biggest));
        ONESHOT_CHK(grow(ix.seg, &d_seg, (size_t)longest * 2));
        std::vector<uint32_t> seg;
        for (const IndexBlock &b : blocks) {
            seg.assign((size_t)b.nq * 2, 0);
            uint32_t at = 0;
            for (uint32_t r = 0; r < b.nq; r++) {
                const uint32_t len = b.nq == 1 ? b.count : tot[b.q0 + r];
                seg[r] = at; seg[b.nq + r] = len; at += len;
            }
            // (a synchronous copy on the null stream: behind the kernels of the block before, which read the segments)
            ONESHOT_CHK(hipMemcpy(d_seg, seg.data(), seg.size() * 4, hipMemcpyHostToDevice));
            const uint32_t *d_start = d_seg, *d_len = d_seg + b.nq;
            ONESHOT_CHK(hipEventRecord(ix.ev[1], nullptr));
            hipLaunchKernelGGL(k_index_probe<1>, dim3(waves_of((size_t)b.nq * B)), dim3(256), 0, nullptr, ix.d_skey, ix.d_sidx, ix.d_keys, n, B,
                               d_qk, b.q0, b.nq, self ? 1u : 0u, (uint32_t *)nullptr, (const uint32_t *)d_off, d_start, d_len, b.lo, d_cp, d_cq);
            ONESHOT_CHK(hipGetLastError());
            ONESHOT_CHK(hipEventRecord(ix.ev[2], nullptr));
            hipLaunchKernelGGL(k_index_verify, dim3((b.count + 3) / 4), dim3(256), 0, nullptr, d_q, ix.d_mins, S, d_cp, d_cq, b.count, d_dist);
            ONESHOT_CHK(hipGetLastError());
            ONESHOT_CHK(hipEventRecord(ix.ev[3], nullptr));
            hipLaunchKernelGGL(k_index_select, dim3((b.nq + 3) / 4), dim3(256), 0, nullptr, d_dist, d_cp, d_start, d_len, b.q0, b.nq, K, lim,
                               d_lkey, d_lidx, d_within);
            ONESHOT_CHK(hipGetLastError());
            ONESHOT_CHK(hipEventRecord(ix.ev[4], nullptr));
            ONESHOT_CHK(hipEventSynchronize(ix.ev[4]));
            ONESHOT_CHK(hipEventElapsedTime(&f, ix.ev[1], ix.ev[2])); ms_probe += f;
            ONESHOT_CHK(hipEventElapsedTime(&f, ix.ev[2], ix.ev[3])); ms_verify += f;
            ONESHOT_CHK(hipEventElapsedTime(&f, ix.ev[3], ix.ev[4])); ms_select += f;
        }
    }
    std::vector<unsigned long long> keys(LK);
    std::vector<uint32_t> within(m);
    ONESHOT_CHK(hipMemcpy(keys.data(), d_lkey, LK * 8, hipMemcpyDeviceToHost));
    ONESHOT_CHK(hipMemcpy(hit_index, d_lidx, LK * 4, hipMemcpyDeviceToHost));
    ONESHOT_CHK(hipMemcpy(within.data(), d_within, (size_t)m * 4, hipMemcpyDeviceToHost));
    uint64_t n_within = 0;
    for (uint32_t i = 0; i < m; i++) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < K; j++) {
            const size_t at = (size_t)i * K + j;
            if (hit_index[at] != 0xFFFFFFFFu) { memcpy(&hit_distance[at], &keys[at], 8); c++; }
            else hit_distance[at] = NAN;
        }
        hit_count[i] = c;
        n_within += within[i];
    }
    if (stats) {
        stats->seconds_total = now_s() - t0; stats->kernel_ms_keys = ms_keys; stats->kernel_ms_probe = ms_probe;
        stats->kernel_ms_verify = ms_verify; stats->kernel_ms_select = ms_select; stats->candidates = candidates; stats->within = n_within;
        stats->query_blocks = n_blocks; stats->pieces = n_pieces;
    }
    return HULK_OK;
}

int hulk_index_search(hulk_index *index, const uint64_t *q_mins, uint32_t m, const hulk_index_search_opts *opts, uint32_t *hit_index,
                      double *hit_distance, uint32_t *hit_count, hulk_index_search_stats *stats) {
    try {
        return index_search(index, q_mins, m, opts, hit_index, hit_distance, hit_count, stats);
    } catch (const std::bad_alloc &) {
        return fail(nullptr, HULK_ERR_HIP, "hulk_index_search: out of host memory");
    }
}

int hulk_index_save(const hulk_index *index, const char *path) {
    if (!index || !path) return fail(nullptr, HULK_ERR_ARG, "hulk_index_save: NULL");
    std::string names;
    for (const std::string &s : index->names) { names += s; names += '\0'; }
    IndexHeader h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, INDEX_MAGIC, 8);
    h.format = INDEX_FORMAT; h.sketch_size = index->S; h.n = index->n; h.bands = index->B;
    memcpy(&h.distance_bits, &index->D, 8);
    h.names_bytes = names.size(); h.mins_bytes = index->mins.size() * 8;
    uint32_t crc = crc32_fast(0, (const uint8_t *)&h, sizeof h);
    crc = crc32_fast(crc, (const uint8_t *)names.data(), names.size());
    crc = crc32_fast(crc, (const uint8_t *)index->mins.data(), (size_t)h.mins_bytes);
    FILE *f = fopen(path, "wb");
    if (!f) return fail(nullptr, HULK_ERR_IO, std::string("hulk_index_save: cannot create ") + path);
    bool ok = fwrite(&h, sizeof h, 1, f) == 1 && (names.empty() || fwrite(names.data(), names.size(), 1, f) == 1) &&
              fwrite(index->mins.data(), (size_t)h.mins_bytes, 1, f) == 1 && fwrite(&crc, 4, 1, f) == 1;
    ok = (fclose(f) == 0) && ok;
    if (!ok) return fail(nullptr, HULK_ERR_IO, std::string("hulk_index_save: cannot write ") + path);
    return HULK_OK;
}

static int index_load(int device, const char *path, hulk_index **index) {
    if (index) *index = nullptr;
    if (!path || !index) return fail(nullptr, HULK_ERR_ARG, "hulk_index_load: NULL");
    const std::string who = std::string("hulk_index_load: ") + path + ": ";
    FILE *f = fopen(path, "rb");
    if (!f) return fail(nullptr, HULK_ERR_IO, who + "cannot open");
    struct Close { FILE *f; ~Close() { fclose(f); } } closer{f};
    IndexHeader h;
    if (fread(&h, sizeof h, 1, f) != 1) return fail(nullptr, HULK_ERR_IO, who + "truncated (no header)");
    if (memcmp(h.magic, INDEX_MAGIC, 8) != 0) return fail(nullptr, HULK_ERR_IO, who + "not a hulk index file");
    if (h.format != INDEX_FORMAT) return fail(nullptr, HULK_ERR_IO, who + "format version " + std::to_string(h.format) + ", this library reads " + std::to_string(INDEX_FORMAT));
    if (fseek(f, 0, SEEK_END) != 0) return fail(nullptr, HULK_ERR_IO, who + "cannot seek");
    const long end = ftell(f);
    if (end < 0 || fseek(f, (long)sizeof h, SEEK_SET) != 0) return fail(nullptr, HULK_ERR_IO, who + "cannot seek");
    const uint64_t size = (uint64_t)end;
    // the lengths the header claims against the file's, before anything is allocated from them
    if (h.n == 0 || h.sketch_size == 0 || h.mins_bytes / 8 / h.sketch_size != h.n || h.mins_bytes != (uint64_t)h.n * h.sketch_size * 8 ||
        h.names_bytes > size || h.mins_bytes > size || sizeof h + h.names_bytes + h.mins_bytes + 4 != size)
        return fail(nullptr, HULK_ERR_IO, who + "truncated or corrupt (the header's lengths do not match the file's " + std::to_string(size) + " bytes)");
    std::string names((size_t)h.names_bytes, '\0');
    std::vector<uint64_t> mins((size_t)h.mins_bytes / 8);
    uint32_t stored = 0;
    if ((h.names_bytes && fread(&names[0], names.size(), 1, f) != 1) || fread(mins.data(), (size_t)h.mins_bytes, 1, f) != 1 || fread(&stored, 4, 1, f) != 1)
        return fail(nullptr, HULK_ERR_IO, who + "truncated");
    uint32_t crc = crc32_fast(0, (const uint8_t *)&h, sizeof h);
    crc = crc32_fast(crc, (const uint8_t *)names.data(), names.size());
    crc = crc32_fast(crc, (const uint8_t *)mins.data(), (size_t)h.mins_bytes);
    if (crc != stored) return fail(nullptr, HULK_ERR_IO, who + "corrupt (checksum mismatch)");
    std::vector<std::string> list;
    for (size_t at = 0; at < names.size();) {
        const size_t z = names.find('\0', at);
        if (z == std::string::npos) return fail(nullptr, HULK_ERR_IO, who + "corrupt (names)");
        list.emplace_back(names, at, z - at);
        at = z + 1;
    }
    if (list.size() != h.n) return fail(nullptr, HULK_ERR_IO, who + "corrupt (" + std::to_string(list.size()) + " names for " + std::to_string(h.n) + " sketches)");
    double D = 0.0;
    memcpy(&D, &h.distance_bits, 8);
    uint32_t B = 0;
    if (h.bands == 0 || index_shape("hulk_index_load", h.n, h.sketch_size, D, h.bands, &B) != HULK_OK)
        return fail(nullptr, HULK_ERR_IO, who + "corrupt (threshold or bands)");
    return index_make(device, std::move(mins), h.n, h.sketch_size, D, B, std::move(list), index);
}

int hulk_index_load(int device, const char *path, hulk_index **index) {
    try {
        return index_load(device, path, index);
    } catch (const std::bad_alloc &) {
        if (index) *index = nullptr;
        return fail(nullptr, HULK_ERR_HIP, "hulk_index_load: out of host memory");
    }
}

}  // extern "C"
