// hulk_oneshot.h — what the entry points that run without a context share (hulk_smash_ex, hulk_panel_distances, hulk_search,
// hulk_cluster, hulk_dendrogram; hulk_set_panel for its temporaries): choosing the device, owning what the call allocates, and the way from host
// sketches to the prepared slot-major arrays.  Helpers, not a framework: every caller keeps its own control flow.
#pragma once
#include "hulk_ctx.h"

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
// (bottomk_view, hulk_bottomk_tile.h, over smash_padded_n(n) rows).  No weights
inline hipError_t upload_bottomk(hipStream_t s, const uint64_t *mins, uint32_t n, uint32_t S, unsigned long long *d_raw_m, double *d_mT,
                                 double *d_wT) {
    hipError_t e = hipMemcpy(d_raw_m, mins, (size_t)n * S * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_bottomk_prep(s, d_raw_m, n, S, d_mT, d_wT);
    return e;
}

}  // namespace hulk
