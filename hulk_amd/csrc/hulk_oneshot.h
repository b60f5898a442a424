// hulk_oneshot.h — what the entry points that run without a context share (hulk_smash_ex, hulk_panel_distances, hulk_search,
// hulk_cluster, hulk_links, hulk_dendrogram, hulk_linkage; hulk_set_panel for its temporaries): choosing the device, owning what the
// call allocates, the way from host sketches to the prepared sets and the kernels' view of them, and the argument checks the
// collection commands share.  Helpers, not a framework: every caller keeps its own control flow.
#pragma once
#include "hulk_ctx.h"
#include "hulk_bottomk_tile.h"

#include <algorithm>

namespace hulk {

// `return` the status of a failed HIP call of a function without a context (the text names the call)
#define ONESHOT_CHK(call) HIPCHK((hulk_ctx *)nullptr, call)

// HULK_OK with `device` the calling thread's current device
inline int oneshot_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, HULK_ERR_NO_DEVICE);
    if (device < 0 || device >= ndev) return fail(nullptr, HULK_ERR_ARG, "device ordinal");
    ONESHOT_CHK(hipSetDevice(device));
    return HULK_OK;
}

// Owns the device buffers and events a call creates: whatever is left when the scope ends — a `return` anywhere — is freed /
// destroyed there.  release(): an early free (the pointer is set to nullptr).
struct OneShot {
    std::vector<void *> bufs;
    std::vector<hipEvent_t> events;
    OneShot() = default;
    OneShot(const OneShot &) = delete;
    OneShot &operator=(const OneShot &) = delete;
    ~OneShot() { for (void *p : bufs) hipFree(p); for (hipEvent_t e : events) hipEventDestroy(e); }
    template <typename T> hipError_t alloc(T **p, size_t count) { const hipError_t e = hipMalloc((void **)p, count * sizeof(T)); if (e == hipSuccess) bufs.push_back(*p); return e; }
    hipError_t event(hipEvent_t *ev) { const hipError_t e = hipEventCreate(ev); if (e == hipSuccess) events.push_back(*ev); return e; }
    template <typename T> hipError_t release(T *&p) { bufs.erase(std::remove(bufs.begin(), bufs.end(), (void *)p), bufs.end()); const hipError_t e = hipFree(p); p = nullptr; return e; }
};

// n host sketches [n][S] -> the raw staging d_raw_m / d_raw_w (n * S entries each, or more) -> k_smash_prep on stream `s` ->
// slot-major d_mT / d_wT [S][smash_padded_n(n)].  The copies are synchronous hipMemcpys: they run behind whatever the null
// stream holds, so a staging buffer the previous launch on the null stream still reads may be passed again.
inline hipError_t upload_prepared(hipStream_t s, const uint64_t *mins, const double *weights, uint32_t n, uint32_t S,
                                  unsigned long long *d_raw_m, double *d_raw_w, double *d_mT, double *d_wT) {
    const size_t bytes = (size_t)n * S * 8;
    hipError_t e = hipMemcpy(d_raw_m, mins, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_raw_w, weights, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_panel_prep(s, d_raw_m, d_raw_w, n, S, d_mT, d_wT);
    return e;
}

// the same for HULK_METRIC_BOTTOMK: n host sketches [n][S] -> d_raw_m -> k_bottomk_prep -> the sorted run-length form in d_mT / d_wT
// (BottomkSet::view, hulk_bottomk_tile.h, over smash_padded_n(n) rows).  No weights
inline hipError_t upload_bottomk(hipStream_t s, const uint64_t *mins, uint32_t n, uint32_t S, unsigned long long *d_raw_m, double *d_mT,
                                 double *d_wT) {
    hipError_t e = hipMemcpy(d_raw_m, mins, (size_t)n * S * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_bottomk_prep(s, d_raw_m, n, S, d_mT, d_wT);
    return e;
}

// upload_bottomk or upload_prepared, as the metric asks
inline hipError_t upload_set(hipStream_t s, int metric, const uint64_t *mins, const double *weights, uint32_t n, uint32_t S,
                             unsigned long long *d_raw_m, double *d_raw_w, double *d_mT, double *d_wT) {
    if (metric == HULK_METRIC_BOTTOMK) return upload_bottomk(s, mins, n, S, d_raw_m, d_mT, d_wT);
    return upload_prepared(s, mins, weights, n, S, d_raw_m, d_raw_w, d_mT, d_wT);
}

// the resident set of hulk_cluster, hulk_links and hulk_dendrogram: d_mT / d_wT [S][smash_padded_n(N)], owned by `own`, prepared from
// the N host sketches.  The raw staging (16 * S bytes a sketch, bottomk's unused weights half included) is freed behind the
// preparation, so the peak of device memory is 32 * S * N bytes and whatever the caller allocated before.  HULK_OK or the status
inline int prepare_set(OneShot &own, int metric, const uint64_t *mins, const double *weights, uint32_t N, uint32_t S, double *&d_mT,
                       double *&d_wT) {
    const size_t NS = (size_t)N * S, NT = (size_t)smash_padded_n(N) * S;
    unsigned long long *d_raw_m = nullptr; double *d_raw_w = nullptr;
    ONESHOT_CHK(own.alloc(&d_mT, NT)); ONESHOT_CHK(own.alloc(&d_wT, NT));
    ONESHOT_CHK(own.alloc(&d_raw_m, NS)); ONESHOT_CHK(own.alloc(&d_raw_w, NS));
    ONESHOT_CHK(upload_set(nullptr, metric, mins, weights, N, S, d_raw_m, d_raw_w, d_mT, d_wT));
    ONESHOT_CHK(hipDeviceSynchronize());
    ONESHOT_CHK(own.release(d_raw_m));
    ONESHOT_CHK(own.release(d_raw_w));
    return HULK_OK;
}

// f(set): the kernels' view of the prepared set in d_mT / d_wT over `rows` rows under `metric` — BottomkSet, PairSet<1> or
// PairSet<0> — so that a launch site names its kernel once, as k_X<decltype(set)>.  A second set of the same type: SET::view,
// which the kernels over one set call themselves: at their launch sites (cluster, links, dendrogram) `set` is there for its TYPE
// only — the kernel is passed d_mT, d_wT and rows and builds the same view again (why: k_dendro_offer, hulk_dendrogram.hip).
// hulk_search passes the values
template <class F>
void with_set(int metric, double *d_mT, double *d_wT, uint32_t rows, uint32_t S, F &&f) {
    if (metric == HULK_METRIC_BOTTOMK) f(BottomkSet::view(d_mT, d_wT, rows, S));
    else if (metric == HULK_METRIC_WEIGHTED_JACCARD) f(PairSet<1>::view(d_mT, d_wT, rows, S));
    else f(PairSet<0>::view(d_mT, d_wT, rows, S));
}

// the opening argument checks of the collection commands (hulk_cluster, hulk_links, hulk_dendrogram, hulk_linkage), in this order:
// NULL pointers (`outputs`: the command's are all there; bottomk reads no weights), n and sketch_size positive, n at most max_n,
// the metric, bottomk's sketch size.  HULK_OK or HULK_ERR_ARG with `fn` in the text
template <class OPTS>
int collection_args(const char *fn, const uint64_t *mins, const double *weights, const OPTS *opts, bool outputs, uint32_t n,
                    uint32_t sketch_size, uint32_t max_n) {
    const std::string f = fn;
    const bool bottomk = opts && opts->metric == HULK_METRIC_BOTTOMK;
    if (!mins || (!weights && !bottomk) || !opts || !outputs) return fail(nullptr, HULK_ERR_ARG, f + ": NULL");
    if (n == 0 || sketch_size == 0) return fail(nullptr, HULK_ERR_ARG, f + ": n and sketch_size must be positive");
    if (n > max_n) return fail(nullptr, HULK_ERR_ARG, f + ": n must be at most " + std::to_string(max_n));
    if (!pair_metric_ok(opts->metric)) return fail(nullptr, HULK_ERR_ARG, f + ": metric");
    if (!bottomk_size_ok(opts->metric, sketch_size))
        return fail(nullptr, HULK_ERR_ARG, f + ": bottomk takes a sketch_size of at most " + std::to_string(HULK_MINHASH_MAX_SKETCH));
    return HULK_OK;
}

// ... and their closing pair: flags outside `allowed`, then the reserved fields
template <class OPTS>
int collection_flags(const char *fn, const OPTS *opts, uint32_t allowed) {
    if (opts->flags & ~allowed) return fail(nullptr, HULK_ERR_ARG, std::string(fn) + ": unknown flags");
    for (uint64_t x : opts->reserved) if (x) return fail(nullptr, HULK_ERR_ARG, std::string(fn) + ": reserved fields must be zero");
    return HULK_OK;
}

}  // namespace hulk
