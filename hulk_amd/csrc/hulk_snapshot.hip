// hulk_snapshot.hip — sketch snapshots (hulk_set_snapshots ... in include/hulk_hip.h): the histosketch as it stands after a
// flushed spectrum, recorded inside the batched flush.  The reference's `--stream` promises "the sketches after every interval"
// (cmd/sketch.go:56) and never reads the flag in src/pipeline; here the states k_cws_apply_snap / k_cws_resolve_drift walk
// through anyway are stored into a device ring, so a caller can watch the sketch evolve without giving up the batch.
//   host knowledge   which spectra of a flush are snapshot points and where they land in the ring (snap_plan, by value in
//                    FlushBatch): no device counters
//   the ring         [cap][sketch_size] mins / weights on the device; snapshot i lives in entry i % cap
//   delivery         hulk_get_snapshots (synchronises), or a callback: behind the kernels of a flush that recorded snapshots the
//                    flush stream copies their entries into a pinned mirror and records an event; the entry points of the step
//                    path query the events of the queued flushes and hand what has arrived to the callback from the mirror
//   the panel        hulk_set_panel: reference sketches held on the device slot-major; behind the kernels of a flush that recorded
//                    snapshots k_snap_panel (hulk_pairwise.hip) scores them against it into a distance ring [cap][n_panel] that
//                    shares the snapshot ring's indices, mirror and delivery
#include "hulk_oneshot.h"

#include <algorithm>

namespace hulk {

constexpr uint32_t SNAP_DEFAULT_CAP = 64;

static int snap_failed(hulk_ctx *c) { return fail(c, HULK_ERR_STATE, "snapshot callback failed"); }

int snap_refuse(hulk_ctx *c, const char *entry) {
    if (!c->snap.every) return HULK_OK;
    return fail(c, HULK_ERR_STATE, std::string(entry) + " is not available on a context that records snapshots (hulk_set_snapshots)");
}

static void panel_teardown(hulk_ctx *c) {
    hulk_ctx::Snapshots::Panel &P = c->snap.panel;
    hipFree(P.d_mT); hipFree(P.d_wT); hipFree(P.d_dist);
    if (P.h_dist) hipHostFree(P.h_dist);
    P = hulk_ctx::Snapshots::Panel{};
}

void snap_teardown(hulk_ctx *c) {
    hulk_ctx::Snapshots &S = c->snap;
    panel_teardown(c);
    hipFree(S.d_mins); hipFree(S.d_weights);
    if (S.h_mins) hipHostFree(S.h_mins);
    if (S.h_weights) hipHostFree(S.h_weights);
    for (size_t i = S.group_head; i < S.groups.size(); i++) hipEventDestroy(S.groups[i].ev);
    for (hipEvent_t e : S.free_events) hipEventDestroy(e);
    S = hulk_ctx::Snapshots{};
}

// the oldest queued flush's snapshots -> the callback; wait == false: only if its event has passed (*ready says whether it had)
static int deliver_front(hulk_ctx *c, bool wait, bool *ready, uint32_t *count) {
    hulk_ctx::Snapshots &S = c->snap;
    hulk_ctx::Snapshots::Group &g = S.groups[S.group_head];
    *ready = true;
    if (wait) HIPCHK(c, hipEventSynchronize(g.ev));
    else {
        const hipError_t e = hipEventQuery(g.ev);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); *ready = false; return HULK_OK; }
        if (e != hipSuccess) return fail_hip(c, e, "hipEventQuery(snapshot)");
    }
    const size_t SS = c->S;
    for (uint32_t i = 0; i < g.n; i++) {
        const size_t at = (size_t)((g.first + i) % S.cap);
        const int r = S.pfn ? S.pfn(S.user, &S.info[at], S.h_mins + at * SS, S.h_weights + at * SS, c->S,
                                    S.panel.n ? S.panel.h_dist + at * S.panel.n : nullptr, S.panel.n)
                            : S.fn(S.user, &S.info[at], S.h_mins + at * SS, S.h_weights + at * SS, c->S);
        S.delivered++;
        if (count) (*count)++;
        if (r != 0) { S.fn_failed = true; c->sticky = HULK_ERR_STATE; return snap_failed(c); }
    }
    S.free_events.push_back(g.ev);
    S.group_head++;
    if (S.group_head == S.groups.size()) { S.groups.clear(); S.group_head = 0; }
    return HULK_OK;
}

int snap_deliver(hulk_ctx *c, bool wait, uint32_t *delivered) {
    hulk_ctx::Snapshots &S = c->snap;
    if (delivered) *delivered = 0;
    if (S.fn_failed) return snap_failed(c);
    if (!S.has_fn()) return HULK_OK;
    while (S.group_head < S.groups.size()) {
        bool ready = false;
        const int rc = deliver_front(c, wait, &ready, delivered);
        if (rc != HULK_OK) return rc;
        if (!ready) break;
    }
    return HULK_OK;
}

int snap_plan(hulk_ctx *c, FlushBatch &fb, uint32_t count, int closed_by, uint64_t *first, uint32_t *n) {
    hulk_ctx::Snapshots &S = c->snap;
    *first = S.recorded; *n = 0;
    if (S.fn_failed) return snap_failed(c);
    const uint64_t I = c->p.interval;
    hulk_snapshot_info infos[SCAN_BATCH_MAX + 1];
    uint32_t mask = 0, k = 0;
    if (count > (uint32_t)SCAN_BATCH_MAX) return fail(c, HULK_ERR_ARG, "batch count");
    for (uint32_t t = 0; t < count; t++) {
        // reads of the stream when spectrum t closed: under the interval rule the flush comes after the whole call was binned
        uint64_t reads = c->seq_count;
        if (closed_by == FLUSH_INTERVAL && I) reads = (c->seq_count - c->seq_count % I) - (uint64_t)(count - 1 - t) * I;
        bool point;
        if (closed_by == FLUSH_EOF) {
            if (reads != S.reads_at_flush) S.ordinal++;          // (an empty last spectrum is flushed, as in the reference, but not counted)
            point = reads != S.reads_at_snapshot;               // whatever its ordinal; a stream that ended on a recorded boundary: no duplicate
        } else {
            S.ordinal++;
            point = S.ordinal % S.every == 0;
        }
        S.reads_at_flush = reads;
        if (point) { mask |= 1u << t; infos[k].ordinal = S.ordinal; infos[k].n_reads = reads; k++; S.reads_at_snapshot = reads; }
    }
    if (!k) return HULK_OK;
    // (hulk_set_snapshots bounded the batch: k <= cap)  With a callback an undelivered snapshot is never overwritten: the
    // flushes that hold the entries this one takes are waited for and delivered first.  Every earlier flush is queued by now.
    if (S.has_fn()) {
        while (S.delivered + S.cap < S.recorded + k) {
            if (S.group_head >= S.groups.size()) return fail(c, HULK_ERR_STATE, "snapshot ring: undelivered snapshots without a queued flush");
            bool ready = false;
            const int rc = deliver_front(c, true, &ready, nullptr);
            if (rc != HULK_OK) return rc;
        }
    }
    for (uint32_t j = 0; j < k; j++) S.info[(size_t)((S.recorded + j) % S.cap)] = infos[j];
    fb.snap_mask = mask; fb.snap_base = (uint32_t)(S.recorded % S.cap); fb.snap_cap = S.cap;
    S.recorded += k;
    *n = k;
    return HULK_OK;
}

int snap_flush_issued(hulk_ctx *c, hipStream_t s, uint64_t first, uint32_t n) {
    hulk_ctx::Snapshots &S = c->snap;
    if (!S.has_fn() || !n) return HULK_OK;
    const size_t SS = c->S, at = (size_t)(first % S.cap), run = std::min<size_t>(n, S.cap - at);
    if (const size_t PN = S.panel.n) {                           // (k_snap_panel has been queued in front of this: flush_kernels)
        HIPCHK(c, hipMemcpyAsync(S.panel.h_dist + at * PN, S.panel.d_dist + at * PN, run * PN * 8, hipMemcpyDeviceToHost, s));
        if (run < n) HIPCHK(c, hipMemcpyAsync(S.panel.h_dist, S.panel.d_dist, (n - run) * PN * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(c, hipMemcpyAsync(S.h_mins + at * SS, S.d_mins + at * SS, run * SS * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(S.h_weights + at * SS, S.d_weights + at * SS, run * SS * 8, hipMemcpyDeviceToHost, s));
    if (run < n) {                                               // the ring wraps inside this flush
        HIPCHK(c, hipMemcpyAsync(S.h_mins, S.d_mins, (n - run) * SS * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(S.h_weights, S.d_weights, (n - run) * SS * 8, hipMemcpyDeviceToHost, s));
    }
    hipEvent_t ev = nullptr;
    if (!S.free_events.empty()) { ev = S.free_events.back(); S.free_events.pop_back(); }
    else HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const hipError_t e = hipEventRecord(ev, s);
    if (e != hipSuccess) { S.free_events.push_back(ev); return fail_hip(c, e, "hipEventRecord(snapshot)"); }
    S.groups.push_back(hulk_ctx::Snapshots::Group{first, n, ev});
    return HULK_OK;
}

int snap_panel_flush(hulk_ctx *c, hipStream_t s, const FlushBatch &fb) {
    const hulk_ctx::Snapshots &S = c->snap;
    if (!S.panel.n || !fb.snap_mask) return HULK_OK;
    HIPCHK(c, launch_snap_panel(s, S.d_mins, S.d_weights, c->S, fb.snap_base, fb.snap_cap, (uint32_t)__builtin_popcount(fb.snap_mask),
                                S.panel.d_mT, S.panel.d_wT, S.panel.n, S.panel.metric, S.panel.role, S.panel.d_dist));
    return HULK_OK;
}

}  // namespace hulk

using namespace hulk;

extern "C" {

int hulk_set_snapshots(hulk_ctx *c, uint32_t every, uint32_t capacity) {
    if (!c) return HULK_ERR_ARG;
    if (c->seq_count || c->flush_index || c->finished) return fail(c, HULK_ERR_STATE, "snapshots must be set before the first read");
    if (c->comm.kind != 0) return fail(c, HULK_ERR_STATE, "snapshots are not available on a multi-rank context");
    if (c->snap.every) c->T = c->ring_n - 1;                       // (back to the batch size of hulk_create)
    snap_teardown(c);
    if (every == 0) return HULK_OK;
    hulk_ctx::Snapshots &S = c->snap;
    const uint32_t cap = capacity ? capacity : SNAP_DEFAULT_CAP;
    const size_t words = (size_t)cap * (c->S ? c->S : 1);
    auto bail = [&](hipError_t e, const char *what) { const int rc = fail_hip(c, e, what); const std::string msg = c->last_error; snap_teardown(c); c->last_error = msg; return rc; };
    hipError_t e;
    if ((e = hipMalloc((void **)&S.d_mins, words * 8)) != hipSuccess) return bail(e, "hipMalloc(snapshot ring)");
    if ((e = hipMalloc((void **)&S.d_weights, words * 8)) != hipSuccess) return bail(e, "hipMalloc(snapshot ring)");
    if ((e = hipHostMalloc((void **)&S.h_mins, words * 8, hipHostMallocDefault)) != hipSuccess) return bail(e, "hipHostMalloc(snapshot staging)");
    if ((e = hipHostMalloc((void **)&S.h_weights, words * 8, hipHostMallocDefault)) != hipSuccess) return bail(e, "hipHostMalloc(snapshot staging)");
    // every entry starts as the empty sketch (0 / MaxFloat64, histosketch.go:84-87): the kernels only ever write the slots this
    // context owns, the others keep these values as they do in hulk_get_sketch
    for (size_t i = 0; i < words; i++) { S.h_mins[i] = 0; S.h_weights[i] = 1.7976931348623157e308; }
    if ((e = hipMemcpy(S.d_mins, S.h_mins, words * 8, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(snapshot ring)");
    if ((e = hipMemcpy(S.d_weights, S.h_weights, words * 8, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(snapshot ring)");
    S.info.assign(cap, hulk_snapshot_info{0, 0});
    S.every = every; S.cap = cap;
    // one flush never records more snapshots than the ring holds: cap * every consecutive spectra hold at most cap points
    c->T = (uint32_t)std::min<uint64_t>(c->ring_n - 1, (uint64_t)cap * every);
    return HULK_OK;
}

int hulk_set_snapshot_callback(hulk_ctx *c, hulk_snapshot_fn fn, void *user) {
    if (!c) return HULK_ERR_ARG;
    if (!c->snap.every) return fail(c, HULK_ERR_STATE, "the context records no snapshots (hulk_set_snapshots)");
    if (c->seq_count || c->flush_index || c->finished) return fail(c, HULK_ERR_STATE, "the snapshot callback must be set before the first read");
    c->snap.fn = fn; c->snap.pfn = nullptr; c->snap.user = user;
    return HULK_OK;
}

int hulk_set_snapshot_panel_callback(hulk_ctx *c, hulk_snapshot_panel_fn fn, void *user) {
    if (!c) return HULK_ERR_ARG;
    if (!c->snap.every) return fail(c, HULK_ERR_STATE, "the context records no snapshots (hulk_set_snapshots)");
    if (c->seq_count || c->flush_index || c->finished) return fail(c, HULK_ERR_STATE, "the snapshot callback must be set before the first read");
    c->snap.pfn = fn; c->snap.fn = nullptr; c->snap.user = user;
    return HULK_OK;
}

int hulk_set_panel(hulk_ctx *c, const uint64_t *mins, const double *weights, uint32_t n_panel, uint32_t sketch_size, int metric, int role) {
    if (!c) return HULK_ERR_ARG;
    if (!c->snap.every) return fail(c, HULK_ERR_STATE, "the context records no snapshots (hulk_set_snapshots)");
    if (c->seq_count || c->flush_index || c->finished) return fail(c, HULK_ERR_STATE, "the panel must be set before the first read");
    if (n_panel == 0) { panel_teardown(c); return HULK_OK; }
    if (!mins || !weights) return fail(c, HULK_ERR_ARG, "NULL");
    if (!metric_ok(metric)) return fail(c, HULK_ERR_ARG, "metric");
    if (!role_ok(role)) return fail(c, HULK_ERR_ARG, "panel role");
    if (sketch_size != c->S) return fail(c, HULK_ERR_ARG, "sketch length mismatch: " + std::to_string(c->S) + " vs " + std::to_string(sketch_size) + "\n");
    if (n_panel > HULK_PANEL_MAX) return fail(c, HULK_ERR_ARG, "panel of " + std::to_string(n_panel) + " sketches (at most " + std::to_string(HULK_PANEL_MAX) + ")");
    panel_teardown(c);
    hulk_ctx::Snapshots::Panel &P = c->snap.panel;
    const size_t NS = (size_t)n_panel * sketch_size, NT = (size_t)smash_padded_n(n_panel) * sketch_size, ND = (size_t)c->snap.cap * n_panel;
    OneShot own;                                                    // the raw upload; the panel's arrays belong to the context
    unsigned long long *d_m = nullptr; double *d_w = nullptr;
    auto bail = [&](hipError_t e, const char *what) {
        const int rc = fail_hip(c, e, what); const std::string msg = c->last_error;
        panel_teardown(c); c->last_error = msg; return rc;
    };
    hipError_t e;
    if ((e = own.alloc(&d_m, NS)) != hipSuccess) return bail(e, "hipMalloc(panel)");
    if ((e = own.alloc(&d_w, NS)) != hipSuccess) return bail(e, "hipMalloc(panel)");
    if ((e = hipMalloc((void **)&P.d_mT, NT * 8)) != hipSuccess) return bail(e, "hipMalloc(panel)");
    if ((e = hipMalloc((void **)&P.d_wT, NT * 8)) != hipSuccess) return bail(e, "hipMalloc(panel)");
    if ((e = hipMalloc((void **)&P.d_dist, ND * 8)) != hipSuccess) return bail(e, "hipMalloc(panel distances)");
    if ((e = hipHostMalloc((void **)&P.h_dist, ND * 8, hipHostMallocDefault)) != hipSuccess) return bail(e, "hipHostMalloc(panel distances)");
    if ((e = hipMemsetAsync(P.d_dist, 0, ND * 8, c->stream)) != hipSuccess) return bail(e, "hipMemsetAsync(panel distances)");
    if ((e = upload_prepared(c->stream, mins, weights, n_panel, sketch_size, d_m, d_w, P.d_mT, P.d_wT)) != hipSuccess) return bail(e, "upload_prepared(panel)");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize(panel)");
    P.n = n_panel; P.metric = metric; P.role = role;
    return HULK_OK;
}

int hulk_get_snapshot_distances(hulk_ctx *c, uint64_t first, uint32_t n, double *out) {
    if (!c) return HULK_ERR_ARG;
    if (!c->snap.every) return fail(c, HULK_ERR_STATE, "the context records no snapshots (hulk_set_snapshots)");
    if (!c->snap.panel.n) return fail(c, HULK_ERR_STATE, "the context has no panel (hulk_set_panel)");
    { const int rcs = sync_all(c); if (rcs != HULK_OK) return rcs; }
    const hulk_ctx::Snapshots &S = c->snap;
    const uint64_t held = S.recorded > S.cap ? S.recorded - S.cap : 0;
    if (first < held) return fail(c, HULK_ERR_ARG, "snapshot " + std::to_string(first) + " was dropped from the ring (oldest held: " + std::to_string(held) + ")");
    if (first + n > S.recorded) return fail(c, HULK_ERR_ARG, "snapshots [" + std::to_string(first) + ", " + std::to_string(first + n) + ") asked for, " + std::to_string(S.recorded) + " recorded");
    if (!n) return HULK_OK;
    if (!out) return fail(c, HULK_ERR_ARG, "NULL");
    const size_t PN = S.panel.n;
    for (uint32_t i = 0; i < n; ) {
        const size_t at = (size_t)((first + i) % S.cap), run = std::min<size_t>(n - i, S.cap - at);
        HIPCHK(c, hipMemcpyAsync(out + (size_t)i * PN, S.panel.d_dist + at * PN, run * PN * 8, hipMemcpyDeviceToHost, c->stream));
        i += (uint32_t)run;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HULK_OK;
}

int hulk_panel_distances(int device, const uint64_t *snap_mins, const double *snap_weights, uint32_t m, const uint64_t *panel_mins,
                         const double *panel_weights, uint32_t n_panel, uint32_t sketch_size, int metric, int role, double *out) {
    if (!metric_ok(metric)) return fail(nullptr, HULK_ERR_ARG, "metric");
    if (!role_ok(role)) return fail(nullptr, HULK_ERR_ARG, "panel role");
    if (n_panel > HULK_PANEL_MAX) return fail(nullptr, HULK_ERR_ARG, "panel of " + std::to_string(n_panel) + " sketches (at most " + std::to_string(HULK_PANEL_MAX) + ")");
    if (!sketch_size) return fail(nullptr, HULK_ERR_ARG, "sketch_size");
    if (!m || !n_panel) return HULK_OK;
    if (!snap_mins || !snap_weights || !panel_mins || !panel_weights || !out) return fail(nullptr, HULK_ERR_ARG, "NULL");
    if (const int rc = oneshot_device(device)) return rc;
    const size_t S = sketch_size, MS = (size_t)m * S, NS = (size_t)n_panel * S, NT = (size_t)smash_padded_n(n_panel) * S, MP = (size_t)m * n_panel;
    OneShot own;
    unsigned long long *d_sm = nullptr, *d_pm = nullptr; double *d_sw = nullptr, *d_pw = nullptr, *d_mT = nullptr, *d_wT = nullptr, *d_out = nullptr;
    ONESHOT_CHK(own.alloc(&d_sm, MS)); ONESHOT_CHK(own.alloc(&d_sw, MS));
    ONESHOT_CHK(own.alloc(&d_pm, NS)); ONESHOT_CHK(own.alloc(&d_pw, NS));
    ONESHOT_CHK(own.alloc(&d_mT, NT)); ONESHOT_CHK(own.alloc(&d_wT, NT));
    ONESHOT_CHK(own.alloc(&d_out, MP));
    ONESHOT_CHK(hipMemcpy(d_sm, snap_mins, MS * 8, hipMemcpyHostToDevice)); ONESHOT_CHK(hipMemcpy(d_sw, snap_weights, MS * 8, hipMemcpyHostToDevice));
    ONESHOT_CHK(upload_prepared(nullptr, panel_mins, panel_weights, n_panel, sketch_size, d_pm, d_pw, d_mT, d_wT));
    for (uint32_t i = 0; i < m; i += SCAN_BATCH_MAX)              // a flush's worth of snapshots per launch; "ring" = this chunk, no wrap
        ONESHOT_CHK(launch_snap_panel(nullptr, d_sm + (size_t)i * S, d_sw + (size_t)i * S, sketch_size, 0, 0xffffffffu,
                                      std::min<uint32_t>(m - i, SCAN_BATCH_MAX), d_mT, d_wT, n_panel, metric, role, d_out + (size_t)i * n_panel));
    ONESHOT_CHK(hipMemcpy(out, d_out, MP * 8, hipMemcpyDeviceToHost));
    return HULK_OK;
}

int hulk_snapshot_count(hulk_ctx *c, uint64_t *recorded, uint64_t *first_held) {
    if (!c) return HULK_ERR_ARG;
    if (!c->snap.every) return fail(c, HULK_ERR_STATE, "the context records no snapshots (hulk_set_snapshots)");
    const hulk_ctx::Snapshots &S = c->snap;
    if (recorded) *recorded = S.recorded;
    if (first_held) *first_held = S.recorded > S.cap ? S.recorded - S.cap : 0;
    return HULK_OK;
}

int hulk_get_snapshots(hulk_ctx *c, uint64_t first, uint32_t n, hulk_snapshot_info *info, uint64_t *mins, double *weights) {
    if (!c) return HULK_ERR_ARG;
    if (!c->snap.every) return fail(c, HULK_ERR_STATE, "the context records no snapshots (hulk_set_snapshots)");
    { const int rcs = sync_all(c); if (rcs != HULK_OK) return rcs; }
    const hulk_ctx::Snapshots &S = c->snap;
    const uint64_t held = S.recorded > S.cap ? S.recorded - S.cap : 0;
    if (first < held) return fail(c, HULK_ERR_ARG, "snapshot " + std::to_string(first) + " was dropped from the ring (oldest held: " + std::to_string(held) + ")");
    if (first + n > S.recorded) return fail(c, HULK_ERR_ARG, "snapshots [" + std::to_string(first) + ", " + std::to_string(first + n) + ") asked for, " + std::to_string(S.recorded) + " recorded");
    const size_t SS = c->S;
    for (uint32_t i = 0; i < n; ) {
        const size_t at = (size_t)((first + i) % S.cap), run = std::min<size_t>(n - i, S.cap - at);
        if (mins) HIPCHK(c, hipMemcpyAsync(mins + (size_t)i * SS, S.d_mins + at * SS, run * SS * 8, hipMemcpyDeviceToHost, c->stream));
        if (weights) HIPCHK(c, hipMemcpyAsync(weights + (size_t)i * SS, S.d_weights + at * SS, run * SS * 8, hipMemcpyDeviceToHost, c->stream));
        if (info) for (size_t j = 0; j < run; j++) info[i + j] = S.info[at + j];
        i += (uint32_t)run;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HULK_OK;
}

int hulk_poll_snapshots(hulk_ctx *c, uint32_t *delivered) {
    if (!c) return HULK_ERR_ARG;
    if (delivered) *delivered = 0;
    if (!c->snap.every) return fail(c, HULK_ERR_STATE, "the context records no snapshots (hulk_set_snapshots)");
    { const int rcf = fatal_status(c); if (rcf != HULK_OK) return rcf; }
    return snap_deliver(c, false, delivered);
}

}  // extern "C"
