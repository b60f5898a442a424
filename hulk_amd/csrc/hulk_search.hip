// hulk_search.hip — nearest-neighbour search of sketches against a database (hulk_search): for every query the K closest database
// sketches, HULKdata.GetDistance exactly as k_smash (hulk_pairwise.hip) computes it, without an M x P array anywhere.
//   the queries     prepared once, slot-major doubles qmT / qwT [slot][QP] (k_smash_prep's layout: (double)min and |w|, zero rows
//                   behind M; QP = M rounded up to 64), resident for the call
//   the database    streams through the device in strips of Pb sketches: upload -> k_smash_prep -> per block of Mb queries
//                   k_search_dist (distances of the block x the strip into the scratch [Mb][Pb]) -> k_search_select (the
//                   running lists of the block's queries).  Device memory: the queries + scratch_bytes, whatever n_db is
//   k_search_dist   the pair tile of hulk_pairtile.h (k_smash's loop: a workgroup of 128 threads owns 32 subjects x 64 others, 16
//                   accumulators a thread that add in slot order; layout and contract are written there) over two different sets.
//                   The SUBJECT side supplies mins, |w| and the union, the other side mins only: ROLE row = the queries are the
//                   subjects, ROLE column = the strip's sketches are (for jaccard the two are one kernel).  Tails in M, P and S
//                   are zero rows / columns as in k_smash; nothing outside block x strip is written.  One template over the set
//                   type: PairSet<0>, PairSet<1> in both roles, BottomkSet (symmetric: ROLE row only)
//   k_search_select a wave owns a query: lane l < K holds entry l of its list, sorted by the 96-bit key (distance bits, database
//                   index) — a non-negative, non-NaN double orders like its uint64 bits.  It reads the strip's row 64 values at
//                   a time (coalesced, eight such loads in flight), rejects against the K-th key (after the first strip nearly everything fails this one
//                   compare), takes the survivors of a ballot in lane order and inserts each (select_insert, hulk_select.h: its rank
//                   in the list is a ballot's population count, the tail moves up one lane).  The compare is the full key, so the
//                   list is a function of the set of pairs alone: no atomics, no appends, no dependence on strips, blocks or scheduling
#include "hulk_oneshot.h"
#include "hulk_pairtile.h"
#include "hulk_bottomk_tile.h"
#include "hulk_select.h"

#include <algorithm>
#include <cmath>

namespace hulk {
namespace {

constexpr int SELECT_AHEAD = 8;

// a: the subject side, columns a0 .. a0 + na of it; b: the other side, columns b0 .. b0 + nb (PairSet: slot-major [S][pitch];
// BottomkSet: rows of the prepared lists, symmetric, so the queries are always a and the rows of `out`).
// out[q][p], pitch doubles per query row: COLUMN 0 the subjects are the queries (q = a, p = b), COLUMN 1 the others are.
// Columns behind na / nb inside a tile are read (the arrays are padded: see hulk_search) and never written.
// search_dist is the kernel's text, a function under k_search_dist: as the kernel's own body hipcc compiles it to other code (k_dendro_offer, hulk_dendrogram.hip)
template <class SET, int COLUMN>
__device__ __forceinline__ void search_dist(const SET a, uint32_t a0, uint32_t na, const SET b, uint32_t b0, uint32_t nb, uint32_t S,
                                            double *__restrict__ out, uint32_t pitch) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;     // other quad, subject quad inside the tile
    const uint32_t s0 = blockIdx.y * PAIR_TS, q0 = blockIdx.x * PAIR_TQ;        // tile origin, relative to a0 / b0
    double acc[4][4], uni[4];
    uint32_t cnt[4][4];
    a.tile(a0 + s0, b, b0 + q0, S, acc, uni, cnt);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t s = s0 + 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t q = q0 + 4 * tx + j;
            if (s < na && q < nb) out[COLUMN ? (size_t)q * pitch + s : (size_t)s * pitch + q] = pair_distance<SET::METRIC>(acc[i][j], uni[i], cnt[i][j], S);
        }
    }
}

template <class SET, int COLUMN>
__global__ __launch_bounds__(128) void k_search_dist(const SET a, uint32_t a0, uint32_t na, const SET b, uint32_t b0, uint32_t nb, uint32_t S,
                                                     double *__restrict__ out, uint32_t pitch) {
    search_dist<SET, COLUMN>(a, a0, na, b, b0, nb, S, out, pitch);
}

// dist [mq][pitch]: row r = query qbase + r against database sketches pbase .. pbase + np.  lkey / lidx [M][K]: the running lists,
// ascending by (distance bits, index), unused entries ~0 / ~0 (behind every key a pair can have).  lim: +Inf = no limit.
__global__ __launch_bounds__(256) void k_search_select(const double *__restrict__ dist, uint32_t pitch, uint32_t mq, uint32_t np,
                                                       uint32_t qbase, uint32_t pbase, uint32_t K, double lim, uint32_t self,
                                                       unsigned long long *__restrict__ lkey, uint32_t *__restrict__ lidx) {
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= mq) return;                                            // (wave-uniform)
    const uint32_t q = qbase + r;
    const double *row = dist + (size_t)r * pitch;
    unsigned long long kd = lane < K ? lkey[(size_t)q * K + lane] : ~0ull;
    uint32_t ki = lane < K ? lidx[(size_t)q * K + lane] : ~0u;
    unsigned long long td = __shfl(kd, (int)K - 1);                 // the K-th key: what a candidate has to beat
    uint32_t ti = __shfl(ki, (int)K - 1);
    for (uint32_t c0 = 0; c0 < np; c0 += 64 * SELECT_AHEAD) {
        double dv[SELECT_AHEAD];                                    // SELECT_AHEAD loads in flight: a wave alone hides no latency
#pragma unroll
        for (int u = 0; u < SELECT_AHEAD; u++) { const uint32_t c = c0 + 64 * u + lane; dv[u] = c < np ? row[c] : lim; }
#pragma unroll
        for (int u = 0; u < SELECT_AHEAD; u++) {
            const uint32_t c = c0 + 64 * u + lane, gi = pbase + c;
            const double d = dv[u];
            const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
            // (d <= lim is false for a NaN; distances are in [0, 1], so the bits order as the values do)
            const bool ok = c < np && d >= 0.0 && d <= lim && !(self && gi == q) && select_beats(bits, gi, td, ti);
            select_insert(__ballot(ok), bits, gi, lane, K, kd, ki, td, ti);      // survivors in lane order = ascending index
        }
    }
    if (lane < K) { lkey[(size_t)q * K + lane] = kd; lidx[(size_t)q * K + lane] = ki; }
}

constexpr uint64_t SEARCH_DEFAULT_SCRATCH = 1ull << 30;
constexpr uint32_t SEARCH_MAX_MB = 2048, SEARCH_MAX_PB = 1u << 20;   // (Pb / 32 and Mb / 32 are grid.y of k_search_dist)

// the scratch holds one strip of Pb database sketches raw and prepared (32 * S bytes a sketch) and the distances [Mb][Pb]
bool search_plan(uint32_t m, uint64_t n_db, uint32_t S, uint64_t scratch_bytes, uint32_t *Mb_out, uint32_t *Pb_out) {
    const uint64_t budget = scratch_bytes ? scratch_bytes : SEARCH_DEFAULT_SCRATCH;
    uint64_t Mb = std::min<uint64_t>(((uint64_t)m + 31) / 32 * 32, SEARCH_MAX_MB), Pb = 0;
    for (;;) {
        Pb = budget / ((uint64_t)S * 32 + Mb * 8) / 64 * 64;
        if (Pb >= 64 || Mb == 32) break;
        Mb = std::max<uint64_t>(32, Mb / 2 / 32 * 32);
    }
    if (Pb < 64) return false;
    Pb = std::min<uint64_t>(Pb, std::min<uint64_t>((n_db + 63) / 64 * 64, SEARCH_MAX_PB));
    *Mb_out = (uint32_t)Mb; *Pb_out = (uint32_t)Pb;
    return true;
}

}  // namespace
}  // namespace hulk

using namespace hulk;

extern "C" int hulk_search(int device, const uint64_t *q_mins, const double *q_weights, uint32_t m, const uint64_t *db_mins,
                           const double *db_weights, uint32_t n_db, uint32_t sketch_size, const hulk_search_opts *opts,
                           uint32_t *hit_index, double *hit_distance, uint32_t *hit_count, hulk_search_stats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    // (HULK_METRIC_BOTTOMK reads no weights: they may be NULL)
    const bool bottomk = opts && opts->metric == HULK_METRIC_BOTTOMK;
    if (!q_mins || (!q_weights && !bottomk) || !opts || !hit_index || !hit_distance || !hit_count) return fail(nullptr, HULK_ERR_ARG, "hulk_search: NULL");
    const uint32_t K = opts->k;
    if (K == 0 || K > HULK_SEARCH_MAX_K) return fail(nullptr, HULK_ERR_ARG, "hulk_search: k must be 1 .. " + std::to_string(HULK_SEARCH_MAX_K));
    if (!pair_metric_ok(opts->metric)) return fail(nullptr, HULK_ERR_ARG, "hulk_search: metric");
    if (!role_ok(opts->role)) return fail(nullptr, HULK_ERR_ARG, "hulk_search: role");
    if (opts->flags & ~HULK_SEARCH_SELF) return fail(nullptr, HULK_ERR_ARG, "hulk_search: unknown flags");
    for (uint64_t x : opts->reserved) if (x) return fail(nullptr, HULK_ERR_ARG, "hulk_search: reserved fields must be zero");
    const bool self = (opts->flags & HULK_SEARCH_SELF) != 0;
    if (self && (db_mins || db_weights)) return fail(nullptr, HULK_ERR_ARG, "hulk_search: HULK_SEARCH_SELF takes no database");
    if (!self && (!db_mins || (!db_weights && !bottomk))) return fail(nullptr, HULK_ERR_ARG, "hulk_search: no database (and no HULK_SEARCH_SELF)");
    if (self) { db_mins = q_mins; db_weights = q_weights; n_db = m; }
    if (m == 0 || n_db == 0 || sketch_size == 0) return fail(nullptr, HULK_ERR_ARG, "hulk_search: m, n_db and sketch_size must be positive");
    const uint32_t S = sketch_size;
    if (!bottomk_size_ok(opts->metric, S)) return fail(nullptr, HULK_ERR_ARG, "hulk_search: bottomk takes a sketch_size of at most " + std::to_string(HULK_MINHASH_MAX_SKETCH));
    uint32_t Mb = 0, Pb = 0;
    if (!search_plan(m, n_db, S, opts->scratch_bytes, &Mb, &Pb))
        return fail(nullptr, HULK_ERR_ARG, "hulk_search: scratch_bytes " + std::to_string(opts->scratch_bytes) + " is too small for one tile (" +
                                               std::to_string(64ull * ((uint64_t)S * 32 + 32 * 8)) + " bytes at this sketch size)");
    const double t0 = now_s();
    if (const int rc = oneshot_device(device)) return rc;
    const double lim = (opts->max_distance >= 0.0 && opts->max_distance <= 1.0) ? opts->max_distance : INFINITY;
    const int metric = opts->metric, column = metric == HULK_METRIC_WEIGHTED_JACCARD && opts->role == HULK_PANEL_COLUMN;
    const uint32_t QP = smash_padded_n(m), DP = smash_padded_n(Pb);
    // (+ 64: with query blocks of 32 a 64-wide tile of ROLE column starts in the middle of the last 64 columns and reads up to 32
    // doubles past a slot's row — the next slot's, or these behind the last one; such columns are computed and never stored)
    const size_t QT = (size_t)QP * S + 64, DT = (size_t)DP * S, MS = (size_t)m * S, LK = (size_t)m * K;
    OneShot own;
    unsigned long long *d_raw_m = nullptr, *d_lkey = nullptr; double *d_raw_w = nullptr, *d_qmT = nullptr, *d_qwT = nullptr, *d_dmT = nullptr, *d_dwT = nullptr, *d_dist = nullptr;
    uint32_t *d_lidx = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    for (hipEvent_t &e : ev) ONESHOT_CHK(own.event(&e));
    // the raw staging serves the queries first, then every strip
    const size_t RAW = std::max(MS, (size_t)Pb * S);
    ONESHOT_CHK(own.alloc(&d_raw_m, RAW)); ONESHOT_CHK(own.alloc(&d_raw_w, RAW));
    ONESHOT_CHK(own.alloc(&d_qmT, QT)); ONESHOT_CHK(own.alloc(&d_qwT, QT));
    ONESHOT_CHK(own.alloc(&d_dmT, DT)); ONESHOT_CHK(own.alloc(&d_dwT, DT));
    ONESHOT_CHK(own.alloc(&d_dist, (size_t)Mb * Pb));
    ONESHOT_CHK(own.alloc(&d_lkey, LK)); ONESHOT_CHK(own.alloc(&d_lidx, LK));
    ONESHOT_CHK(hipMemset(d_lkey, 0xff, LK * 8)); ONESHOT_CHK(hipMemset(d_lidx, 0xff, LK * 4));
    ONESHOT_CHK(hipMemset(d_qmT + (size_t)QP * S, 0, 64 * 8)); ONESHOT_CHK(hipMemset(d_qwT + (size_t)QP * S, 0, 64 * 8));
    // bottomk: the same buffers hold the sorted run-length form (BottomkSet::view), the strips' too
    ONESHOT_CHK(upload_set(nullptr, metric, q_mins, q_weights, m, S, d_raw_m, d_raw_w, d_qmT, d_qwT));
    double ms_dist = 0.0, ms_select = 0.0;
    uint32_t strips = 0, blocks = 0;
    for (uint64_t p0 = 0; p0 < n_db; p0 += Pb, strips++) {
        const uint32_t np = (uint32_t)std::min<uint64_t>(Pb, n_db - p0);
        // (hipMemcpy on the null stream: behind the kernels that read the previous strip)
        const double *db_w = db_weights ? db_weights + (size_t)p0 * S : nullptr;        // (bottomk: may be NULL)
        ONESHOT_CHK(upload_set(nullptr, metric, db_mins + (size_t)p0 * S, db_w, np, S, d_raw_m, d_raw_w, d_dmT, d_dwT));
        const uint32_t NP = smash_padded_n(np);                     // the pitch k_smash_prep gave this strip
        blocks = 0;
        for (uint32_t qb = 0; qb < m; qb += Mb, blocks++) {
            const uint32_t mq = std::min(Mb, m - qb);
            ONESHOT_CHK(hipEventRecord(ev[0], nullptr));
            with_set(metric, d_qmT, d_qwT, QP, S, [&](auto qs) {
                using SET = decltype(qs);
                const SET ds = SET::view(d_dmT, d_dwT, NP, S);
                if constexpr (SET::METRIC == 1) {                   // ROLE column: the strip is the subject side.  The symmetric
                    if (column) {                                   // metrics have no such instance: the role changes nothing
                        hipLaunchKernelGGL((k_search_dist<SET, 1>), dim3((mq + PAIR_TQ - 1) / PAIR_TQ, (np + PAIR_TS - 1) / PAIR_TS), dim3(128), 0,
                                           nullptr, ds, 0u, np, qs, qb, mq, S, d_dist, Pb);
                        return;
                    }
                }
                hipLaunchKernelGGL((k_search_dist<SET, 0>), dim3((np + PAIR_TQ - 1) / PAIR_TQ, (mq + PAIR_TS - 1) / PAIR_TS), dim3(128), 0, nullptr,
                                   qs, qb, mq, ds, 0u, np, S, d_dist, Pb);
            });
            ONESHOT_CHK(hipGetLastError());
            ONESHOT_CHK(hipEventRecord(ev[1], nullptr));
            hipLaunchKernelGGL(k_search_select, dim3((mq + 3) / 4), dim3(256), 0, nullptr, d_dist, Pb, mq, np, qb, (uint32_t)p0, K, lim,
                               self ? 1u : 0u, d_lkey, d_lidx);
            ONESHOT_CHK(hipGetLastError());
            ONESHOT_CHK(hipEventRecord(ev[2], nullptr));
            ONESHOT_CHK(hipEventSynchronize(ev[2]));
            float a = 0, b = 0;
            ONESHOT_CHK(hipEventElapsedTime(&a, ev[0], ev[1])); ONESHOT_CHK(hipEventElapsedTime(&b, ev[1], ev[2]));
            ms_dist += a; ms_select += b;
        }
    }
    std::vector<unsigned long long> keys(LK);
    ONESHOT_CHK(hipMemcpy(keys.data(), d_lkey, LK * 8, hipMemcpyDeviceToHost));
    ONESHOT_CHK(hipMemcpy(hit_index, d_lidx, LK * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < m; i++) {
        uint32_t n = 0;
        for (uint32_t j = 0; j < K; j++) {
            const size_t at = (size_t)i * K + j;
            if (hit_index[at] != 0xFFFFFFFFu) { memcpy(&hit_distance[at], &keys[at], 8); n++; }
            else hit_distance[at] = NAN;
        }
        hit_count[i] = n;
    }
    if (stats) { stats->seconds_total = now_s() - t0; stats->kernel_ms_dist = ms_dist; stats->kernel_ms_select = ms_select; stats->strips = strips; stats->query_blocks = blocks; }
    return HULK_OK;
}
