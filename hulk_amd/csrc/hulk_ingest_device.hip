// The device side of the host ingest (hulk_ingest.h): the sink that hands parsed reads to a context, the device parsers' buffer
// sets and reader thread, the run loops of the device FASTQ and FASTA parsers (hulk_fastq.hip has the kernels) and
// hulk_sketch_files.  Everything here runs on the calling thread but RawReader's thread.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "hulk_ingest.h"
#include "hulk_internal.h"
#include "hulk_fastq.h"
#include "hulk_bgzf.h"

namespace hulk {
namespace ingest {
namespace {

// pinned double-buffered staging in front of hulk_add_reads_device
struct GpuSink : Sink {
    // the staging (two pinned + device sets) is the context's: nothing is allocated or freed per run after the first
    hulk_ctx *ctx; hulk::StageSet st{}; uint64_t min_len; PhaseTrace &g_trace;      // (the run's own trace)
    GpuSink(hulk_ctx *c, PhaseTrace &tr) : ctx(c), min_len(hulk::ctx_min_read_len(c)), g_trace(tr) {}
    bool prepare(uint64_t n, uint64_t nbytes, uint8_t **b, uint64_t **l, IngestError &err) override {
        const double tw0 = PhaseTrace::now();
        const int rc = hulk::ctx_stage_acquire(ctx, (size_t)nbytes, n, &st);
        g_trace.stage_wait += PhaseTrace::now() - tw0;
        if (rc != HULK_OK) return err.set(rc, hulk_last_error(ctx));
        *b = st.h_bases; *l = st.h_off;
        return true;
    }
    bool commit(uint64_t n, IngestError &err) override {
        if (n == 0) return true;
        uint64_t mn, mx;
        const uint64_t tot = lens_to_offsets(st.h_off, n, mn, mx);
        if (!check_read_lengths(mn, mx, min_len, err)) return false;
        hipStream_t stream = hulk::ctx_stream(ctx);
        const double tc0 = PhaseTrace::now();
        ING_HIP(hipMemcpyAsync(st.d_bases, st.h_bases, tot, hipMemcpyHostToDevice, stream));
        ING_HIP(hipMemcpyAsync(st.d_off, st.h_off, (n + 1) * 8, hipMemcpyHostToDevice, stream));
        const double tc1 = PhaseTrace::now(); g_trace.enqueue += tc1 - tc0;
        // (long sequences: their lengths are read from the staged offsets, not fetched back)
        int rc = hulk::add_reads_device(ctx, st.d_bases, st.d_off, n, (uint32_t)mx, st.cap_bases, st.h_off);
        g_trace.add_reads += PhaseTrace::now() - tc1;
        if (rc != HULK_OK) return err.set(rc, hulk_last_error(ctx));
        rc = hulk::ctx_stage_release(ctx);
        if (rc != HULK_OK) return err.set(rc, hulk_last_error(ctx));
        n_seqs += n; total_len += tot;
        return true;
    }
    bool finish(IngestError &) override { return true; }      // (the sets stay the context's; whoever takes one next waits for its event)
};

// the kernels of a context still read a buffer handed to it: two events, recorded behind them on the context's stream and, if
// there is one, on its second work lane.  Whoever writes the buffer next makes its stream wait for them first.
struct BusyPair {
    hipEvent_t ev[2] = {}; bool on[2] = {};
    hipError_t wait(hipStream_t s) {
        for (int i = 0; i < 2; i++)
            if (on[i]) { const hipError_t e = hipStreamWaitEvent(s, ev[i], 0); if (e != hipSuccess) return e; on[i] = false; }
        return hipSuccess;
    }
    int mark(hulk_ctx *ctx) { const int rc = hulk::ctx_record_busy(ctx, ev[0], ev[1], &on[1]); if (rc == HULK_OK) on[0] = true; return rc; }
    void clear() { on[0] = on[1] = false; }
};

// ------------------------------------------------------------------------------------------
// FASTQ -> reads on the DEVICE (hulk_fastq.hip).  The host's part of a run shrinks to moving bytes: a reader thread fills
// pinned buffers with raw file bytes (ByteSource: files, gzip, STDIN — fixed-size blocks, cut anywhere), the calling thread
// queues one host-to-device copy and one chain of parse kernels per block and hands the parsed reads of the block before to
// hulk_add_reads_device.  Streams: copies on `cs`, parse kernels on `ps`, binning on the context's lanes;
//   copy(b) -> parse(b) [after parse(b-1): the tail; after the binning of block b-2 has read the output set] -> the block's
//   scalars reach the host -> hulk_add_reads_device(b) while copy(b+1) / parse(b+1) are already under way.
// Buffers: 6 pinned blocks, 4 raw device blocks (porch + block), 3 output sets (bases + offsets), one set of line-index arrays
// — 6 x 16 MiB = 96 MB pinned and about 300 MB of HBM at the default block size.  They belong to the PROCESS, not to a context: a
// run borrows an idle set for its device and block size and hands it back (a `hulk sketch` per file on fresh contexts would
// otherwise pin and unpin 64 MB per file: tens of milliseconds each).  The pool is bounded in size (FQ_POOL_MAX sets) and in AGE:
// a set nobody borrowed for FQ_IDLE_SECONDS is freed by the next hulk_create / hulk_destroy / hulk_sketch_files of the process
// (fq_sweep_idle), so a host that sketched one file does not hold the buffers for as long as it keeps using the library;
// hulk_release_caches() frees them at once.
// ------------------------------------------------------------------------------------------
struct FqDev {
    // FASTQ keeps DEPTH blocks queued behind the one whose reads it hands over (with one, the PCIe link idled a third of the time:
    // a block's copy was queued only when the parse of the block before the previous one had been waited for): a block's raw slot is
    // its successor's tail source and, should the host parser take over, the successor's successor's — NRAW = DEPTH + 2; an output
    // set is written again when DEPTH blocks behind it have been queued — NOUT = DEPTH + 1
    static constexpr int DEPTH = 2, NRAW = DEPTH + 2, NOUT = DEPTH + 1, NHOST = 6, NST = 6;
    int device = 0; size_t block = 0; uint32_t porch = 0;
    double idle_since = 0.0;                                       // when the set went back to the pool (steady clock, seconds)
    hipStream_t cs = nullptr, ps = nullptr;
    uint8_t *d_raw[NRAW] = {}, *h_buf[NHOST] = {}, *d_bases[NOUT] = {};
    uint64_t *d_off[NOUT] = {};
    hulk::FqState *d_state = nullptr, *h_state = nullptr;          // [NST]
    hipEvent_t ev_copied[NHOST] = {}, ev_parsed[NST] = {};
    BusyPair out_busy[NOUT];                                       // the context's kernels still read output set o
    hulk::FqBuffers B;
    // --fasta (run_ingest_fasta_device), allocated by the first such run of the set: two line indices with room for (64 KiB + block) / 2
    // lines each, two accumulation buffers (sequence bytes of complete records + the record in progress; they grow with the longest
    // record) and their record offsets — about 2 x 135 MB + 2 x (192 MB + 70 MB) of HBM at the default block size
    struct Fasta {
        bool ready = false;
        hulk::FaBuffers B[2];                                      // index arrays: a block is indexed while the one before it is placed
        hipEvent_t ev_placed[NRAW] = {};                           // the block that used raw slot r has been placed (the slot may be overwritten)
        hulk::FaState *d_state = nullptr, *h_state = nullptr;      // [NST]
        uint8_t *acc[2] = {}; size_t acc_cap[2] = {};
        uint64_t *rec_off[2] = {}; size_t rec_cap = 0;
        BusyPair acc_busy[2];                                      // the context's kernels still read records of acc[i]
    } fa;
    // HULK_INGEST_DEVICE_INFLATE (allocated by the first such run of the set): two batches of members and a device twin of each
    // pinned block — about 2 x 144 MB + 6 x 16 MiB of HBM and 2 x 16 MiB pinned at the default block size
    hulk::bgzf::DevBufs *gz = nullptr;
    size_t raw_bytes() const { return (size_t)porch + block + 64; }
    void release() {
        if (cs) hipStreamSynchronize(cs);
        if (ps) hipStreamSynchronize(ps);
        hulk::bgzf::dev_bufs_free(gz); gz = nullptr;
        for (auto &b : fa.B) { hipFree(b.wgcnt); hipFree(b.line_end); hipFree(b.linfo); hipFree(b.ldst); hipFree(b.wghdr); hipFree(b.hrel); hipFree(b.wgbytes); }
        for (auto &e : fa.ev_placed) if (e) hipEventDestroy(e);
        hipFree(fa.d_state); if (fa.h_state) hipHostFree(fa.h_state);
        for (int i = 0; i < 2; i++) { hipFree(fa.acc[i]); hipFree(fa.rec_off[i]); for (auto &e : fa.acc_busy[i].ev) if (e) hipEventDestroy(e); }
        fa = Fasta{};
        for (auto &p : d_raw) { hipFree(p); p = nullptr; }
        for (auto &p : d_bases) { hipFree(p); p = nullptr; }
        for (auto &p : d_off) { hipFree(p); p = nullptr; }
        for (auto &p : h_buf) { if (p) hipHostFree(p); p = nullptr; }
        hipFree(d_state); d_state = nullptr;
        if (h_state) hipHostFree(h_state); h_state = nullptr;
        hipFree(B.wgcnt); hipFree(B.line_end); hipFree(B.linfo); hipFree(B.wgmap); hipFree(B.wgseq); hipFree(B.src_out);
        hipFree(B.lmap); hipFree(B.wgstate); hipFree(B.wgbytes);
        B = hulk::FqBuffers{};
        for (auto &e : ev_copied) { if (e) hipEventDestroy(e); e = nullptr; }
        for (auto &e : ev_parsed) { if (e) hipEventDestroy(e); e = nullptr; }
        for (auto &pr : out_busy) { for (auto &e : pr.ev) if (e) hipEventDestroy(e); pr = BusyPair{}; }
        if (cs) hipStreamDestroy(cs); if (ps) hipStreamDestroy(ps);
        cs = ps = nullptr;
    }
    static void destroy(void *p) { FqDev *d = (FqDev *)p; d->release(); delete d; }
};

// idle buffer sets of the process (at most FQ_POOL_MAX are kept; the others are freed when their run ends)
static std::mutex g_fq_mu;
static std::vector<FqDev *> g_fq_idle;
constexpr size_t FQ_POOL_MAX = 2;
constexpr double FQ_IDLE_SECONDS = 10.0;
static double fq_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void fq_dev_release(FqDev *d) {
    if (!d) return;
    {
        std::lock_guard<std::mutex> g(g_fq_mu);
        if (g_fq_idle.size() < FQ_POOL_MAX) { d->idle_since = fq_now(); g_fq_idle.push_back(d); return; }
    }
    FqDev::destroy(d);
}
}  // namespace
}  // namespace ingest
void fq_release_idle() {
    using namespace ingest;
    std::vector<FqDev *> drop;
    { std::lock_guard<std::mutex> g(g_fq_mu); drop.swap(g_fq_idle); }
    for (FqDev *d : drop) FqDev::destroy(d);
    RegionPool::get().sweep(0.0);
}
// frees the idle sets nobody has borrowed for FQ_IDLE_SECONDS (called from hulk_create / hulk_destroy / hulk_sketch_files)
void fq_sweep_idle() {
    using namespace ingest;
    std::vector<FqDev *> drop;
    {
        std::lock_guard<std::mutex> g(g_fq_mu);
        const double t = fq_now();
        for (size_t i = 0; i < g_fq_idle.size();)
            if (t - g_fq_idle[i]->idle_since > FQ_IDLE_SECONDS) { drop.push_back(g_fq_idle[i]); g_fq_idle.erase(g_fq_idle.begin() + i); }
            else i++;
    }
    for (FqDev *d : drop) FqDev::destroy(d);
    RegionPool::get().sweep(FQ_IDLE_SECONDS);
}
}  // namespace hulk
namespace hulk {
namespace ingest {
namespace {
// the buffers, streams and events of a new set
static bool fq_dev_alloc(FqDev *d, IngestError &err) {
    const size_t block = d->block;
    ING_HIP(hipSetDevice(d->device));
    ING_HIP(hipStreamCreateWithFlags(&d->cs, hipStreamNonBlocking));
    {   // the parse kernels are short and the calling thread waits for their scalars block by block, while the context's lanes keep
        // the chip full with binning kernels: their workgroups go first when CUs come free
        int lo = 0, hi = 0;
        ING_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        ING_HIP(hipStreamCreateWithPriority(&d->ps, hipStreamNonBlocking, hi));
    }
    hulk::FqBuffers &B = d->B;
    B.porch = d->porch;
    B.line_cap = (uint32_t)((d->porch + block) / 8 + 1024);
    B.read_cap = B.line_cap / 2;
    B.bytes_cap = d->porch + block;
    for (auto &p : d->d_raw) { ING_HIP(hipMalloc((void **)&p, d->raw_bytes())); ING_HIP(hipMemset(p, '\n', d->raw_bytes())); }
    for (auto &p : d->h_buf) ING_HIP(hipHostMalloc((void **)&p, block, hipHostMallocDefault));
    for (auto &p : d->d_bases) ING_HIP(hipMalloc((void **)&p, B.bytes_cap + 64));
    for (auto &p : d->d_off) ING_HIP(hipMalloc((void **)&p, ((size_t)B.read_cap + 2) * 8));
    ING_HIP(hipMalloc((void **)&d->d_state, FqDev::NST * sizeof(hulk::FqState)));
    ING_HIP(hipHostMalloc((void **)&d->h_state, FqDev::NST * sizeof(hulk::FqState), hipHostMallocDefault));
    const size_t nchunk = (d->raw_bytes() + 4095) / 4096 + 8, nlwg = ((size_t)B.line_cap + 255) / 256 + 8;      // (hulk_fastq.hip FQ_T = 256)
    ING_HIP(hipMalloc((void **)&B.wgcnt, nchunk * 4));
    ING_HIP(hipMalloc((void **)&B.line_end, (size_t)B.line_cap * 4));
    ING_HIP(hipMalloc((void **)&B.linfo, (size_t)B.line_cap * 4));
    ING_HIP(hipMalloc((void **)&B.lmap, (size_t)B.line_cap));
    ING_HIP(hipMalloc((void **)&B.wgmap, nlwg * 4));
    ING_HIP(hipMalloc((void **)&B.wgstate, nlwg));
    ING_HIP(hipMalloc((void **)&B.wgseq, nlwg * 4));
    ING_HIP(hipMalloc((void **)&B.wgbytes, nlwg * 8));
    ING_HIP(hipMalloc((void **)&B.src_out, ((size_t)B.read_cap + 2) * 4));
    for (auto &e : d->ev_copied) ING_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : d->ev_parsed) ING_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &pr : d->out_busy) for (auto &e : pr.ev) ING_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ING_HIP(hipDeviceSynchronize());
    return true;
}
// a parser for blocks of `block` bytes on the context's device: an idle set of the process, or a new one
static FqDev *fq_dev_for(hulk_ctx *ctx, size_t block, IngestError &err) {
    const int device = hulk::ctx_device(ctx);
    {
        std::lock_guard<std::mutex> g(g_fq_mu);
        for (size_t i = 0; i < g_fq_idle.size(); i++)
            if (g_fq_idle[i]->device == device && g_fq_idle[i]->block == block) {
                FqDev *d = g_fq_idle[i]; g_fq_idle.erase(g_fq_idle.begin() + i); return d;
            }
        // (a set of another shape makes room)
        if (g_fq_idle.size() >= FQ_POOL_MAX) { FqDev::destroy(g_fq_idle.front()); g_fq_idle.erase(g_fq_idle.begin()); }
    }
    FqDev *d = new FqDev();
    d->device = device; d->block = block; d->porch = 1u << 20;
    if (!fq_dev_alloc(d, err)) { FqDev::destroy(d); return nullptr; }
    return d;
}

// reader thread of the device path: raw blocks of exactly `block` bytes (the last one shorter) into the pinned buffers
class RawReader {
 public:
    // dev: [offset, length) pieces of the block that are device text, in the twin of pinned buffer idx (the rest is in the buffer)
    struct Item { int idx = -1; size_t len = 0; bool eof = false; std::vector<std::pair<size_t, size_t>> dev; };
    RawReader(const char *const *paths, uint32_t n, const IngestCfg &cfg, FqDev *dev) : dev_(dev), src_(paths, n, cfg) {
        for (int i = 0; i < FqDev::NHOST; i++) free_.push_back(i);
        if (cfg.dev_inflate) src_.set_device_inflate(dev->gz);
        th_ = std::thread([this] { run(); });
    }
    ~RawReader() {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        cv_.notify_all();
        if (th_.joinable()) th_.join();
    }
    bool next(Item &it, IngestError &err) {                  // false: the stream has ended (or failed: err)
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [this] { return !q_.empty() || done_; });
        if (!q_.empty()) { it = q_.front(); q_.pop_front(); return true; }
        if (err_.code != HULK_OK) err = err_;
        return false;
    }
    void recycle(int idx) { { std::lock_guard<std::mutex> g(m_); free_.push_back(idx); } cv_.notify_all(); }
    uint64_t bytes_in() const { return bytes_in_; }

 private:
    void run() {
        for (;;) {
            int idx;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [this] { return !free_.empty() || stop_; });
                if (stop_) break;
                idx = free_.front(); free_.pop_front();
            }
            size_t have = 0; bool eof = false; IngestError e;
            Item it;
            uint8_t *twin = dev_->gz ? hulk::bgzf::dev_bufs_block(dev_->gz, idx) : nullptr;
            while (have < dev_->block) {
                bool on_dev = false;
                const long n = src_.read(dev_->h_buf[idx] + have, dev_->block - have, e, twin ? twin + have : nullptr, &on_dev);
                if (n < 0) { std::lock_guard<std::mutex> g(m_); err_ = e; done_ = true; cv_.notify_all(); return; }
                if (n == 0) { eof = true; break; }
                if (on_dev) {
                    if (!it.dev.empty() && it.dev.back().first + it.dev.back().second == have) it.dev.back().second += (size_t)n;
                    else it.dev.emplace_back(have, (size_t)n);
                }
                have += (size_t)n; bytes_in_ += (uint64_t)n;
            }
            if (!it.dev.empty() && hulk::bgzf::dev_bufs_mark_block(dev_->gz, idx) != hipSuccess) {
                std::lock_guard<std::mutex> g(m_); err_.set(HULK_ERR_HIP, "hipEventRecord (device BGZF text)"); done_ = true; cv_.notify_all(); return;
            }
            { std::lock_guard<std::mutex> g(m_); it.idx = idx; it.len = have; it.eof = eof; q_.push_back(std::move(it)); }
            cv_.notify_all();
            if (eof) break;
        }
        { std::lock_guard<std::mutex> g(m_); done_ = true; }
        cv_.notify_all();
    }
    FqDev *dev_;
    ByteSource src_;
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<Item> q_;
    std::deque<int> free_;
    bool done_ = false, stop_ = false;
    IngestError err_;
    std::atomic<uint64_t> bytes_in_{0};
};

// HULK_INGEST_DEVICE_INFLATE: the set's device BGZF reader buffers (hulk_bgzf.hip), allocated by the first such run
static bool gz_ensure(FqDev *D, IngestError &err) {
    if (D->gz) return true;
    std::string msg;
    D->gz = hulk::bgzf::dev_bufs_new(D->device, FqDev::NHOST, D->block, msg);
    return D->gz ? true : err.set(HULK_ERR_HIP, msg);
}
// a block's bytes -> its raw slot on the copy stream: pinned bytes host-to-device, device text device-to-device from the
// block's twin (behind the reader thread's copies into it)
static hipError_t copy_block(FqDev *D, const RawReader::Item &it, uint8_t *dst) {
    if (it.dev.empty()) return hipMemcpyAsync(dst, D->h_buf[it.idx], it.len, hipMemcpyHostToDevice, D->cs);
    const uint8_t *twin = hulk::bgzf::dev_bufs_block(D->gz, it.idx);
    hipError_t e = hipStreamWaitEvent(D->cs, hulk::bgzf::dev_bufs_block_event(D->gz, it.idx), 0);
    size_t at = 0;
    for (const auto &pc : it.dev) {
        if (e == hipSuccess && pc.first > at) e = hipMemcpyAsync(dst + at, D->h_buf[it.idx] + at, pc.first - at, hipMemcpyHostToDevice, D->cs);
        if (e == hipSuccess) e = hipMemcpyAsync(dst + pc.first, twin + pc.first, pc.second, hipMemcpyDeviceToDevice, D->cs);
        at = pc.first + pc.second;
    }
    if (e == hipSuccess && it.len > at) e = hipMemcpyAsync(dst + at, D->h_buf[it.idx] + at, it.len - at, hipMemcpyHostToDevice, D->cs);
    return e;
}
// the host parser takes over: a block's device text back into its pinned buffer
static bool host_bytes(FqDev *D, const RawReader::Item &it, IngestError &err) {
    if (it.dev.empty()) return true;
    const uint8_t *twin = hulk::bgzf::dev_bufs_block(D->gz, it.idx);
    if (hipEventSynchronize(hulk::bgzf::dev_bufs_block_event(D->gz, it.idx)) != hipSuccess) return err.set(HULK_ERR_HIP, "hipEventSynchronize (device BGZF text)");
    for (const auto &pc : it.dev)
        if (hipMemcpy(D->h_buf[it.idx] + pc.first, twin + pc.first, pc.second, hipMemcpyDeviceToHost) != hipSuccess)
            return err.set(HULK_ERR_HIP, "hipMemcpy (device BGZF text to the host parser)");
    return true;
}

// ------------------------------------------------------------------------------------------
// What the two device run loops share.  A run borrows a buffer set (DevRun), its reader thread fills pinned blocks, and per block
// the calling thread queues: the copy into a raw slot on `cs` (queue_copy), the parser's kernels on `ps` behind it (the parser's
// own), the block's scalars back to the host and ev_parsed (state_back).  Blocks stay held until their scalars have been taken
// (Pump); what is parsed goes to the context behind the parse stream, and the context's kernels mark the buffer busy (add_parsed).
// The loop around the pump is written out in both runs: what queues a block and what takes its result are the parser's own.
// ------------------------------------------------------------------------------------------
static bool fa_ensure(FqDev *D, IngestError &err);              // (the FASTA parser's part of a set: below, with its run)
struct DevRun {
    hulk_ctx *ctx; PhaseTrace &tr; IngestError &err;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    IngestCfg cfg; FqDev *D = nullptr; uint64_t min_len = 0;
    DevRun(hulk_ctx *c, PhaseTrace &t, IngestError &e) : ctx(c), tr(t), err(e) {}
    // (declared before the reader: the set goes back after the reader's thread has ended)
    ~DevRun() { if (D) { hipStreamSynchronize(D->cs); hipStreamSynchronize(D->ps); fq_dev_release(D); } }
    // The host's whole job is read() into pinned memory and one PCIe copy per block, so its best settings are not the
    // parser's: 16 MiB blocks read in 16 pieces side by side moved 46 GB/s of a page-cached file (1.5e8 reads/s of 150 bp
    // FASTQ: the PCIe link), 4 pieces 33; 8 MiB blocks 28 (profiles/r05_devparse.txt).  A caller's figures are taken as they are
    // (the line index holds (porch + block) / 8 + 1024 lines in workgroups of 256 — 8,708 of them at 16 MiB —, which the one-workgroup
    // scans walk in trips of 2,048: blocks of up to 32 MiB).
    bool begin(const char *const *paths, uint32_t n_paths, const IngestCfg &cfg_in, bool fasta) {
        if (n_paths && !paths) return err.set(HULK_ERR_ARG, "NULL path list");
        cfg = cfg_in;
        if (!cfg.block_set) cfg.block = (size_t)16u << 20;
        if (!cfg.readers_set) { const unsigned hw = std::thread::hardware_concurrency(); cfg.readers = hw ? std::min(16u, hw) : 4u; }
        D = fq_dev_for(ctx, std::min<size_t>(cfg.block, (size_t)32u << 20), err);
        if (!D) return false;
        ING_HIP(hipSetDevice(D->device));
        if (fasta && !fa_ensure(D, err)) return false;
        if (cfg.dev_inflate && !gz_ensure(D, err)) return false;
        min_len = hulk::ctx_min_read_len(ctx);
        return true;
    }
    // nothing of this run may still read the pinned blocks or write the output sets when the next run starts
    void end(const RawReader &reader, hulk_ingest_stats *stats, uint64_t n_seqs, uint64_t total_len, uint64_t n_lines) {
        hipStreamSynchronize(D->cs); hipStreamSynchronize(D->ps);
        if (!stats) return;
        stats->n_seqs = n_seqs; stats->total_len = total_len; stats->n_lines = n_lines;
        stats->bytes_in = reader.bytes_in();
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
};

// block `it` into raw slot r on the copy stream, behind `after` (what last needed the slot's old contents; nullptr: nothing), and
// the parse stream behind the copy
static bool queue_copy(FqDev *D, const RawReader::Item &it, int r, hipEvent_t after, IngestError &err) {
    if (after) ING_HIP(hipStreamWaitEvent(D->cs, after, 0));
    ING_HIP(copy_block(D, it, D->d_raw[r] + D->porch));
    ING_HIP(hipEventRecord(D->ev_copied[it.idx], D->cs));
    ING_HIP(hipStreamWaitEvent(D->ps, D->ev_copied[it.idx], 0));
    return true;
}
// a block's scalars to the host behind its kernels; ev_parsed[st] says when they are there
static bool state_back(FqDev *D, void *h_state, const void *d_state, size_t bytes, int st, IngestError &err) {
    ING_HIP(hipMemcpyAsync(h_state, d_state, bytes, hipMemcpyDeviceToHost, D->ps));
    ING_HIP(hipEventRecord(D->ev_parsed[st], D->ps));
    return true;
}
// n sequences that the parse stream leaves in device buffers -> the context, behind `parsed` (nullptr: nothing to wait for);
// h_off: the host's copy of their offsets, if it has one.  The context's kernels then hold the buffer: `busy`.
static bool add_parsed(DevRun &R, hipEvent_t parsed, const uint8_t *d_bases, const uint64_t *d_off, uint64_t n, uint32_t max_len,
                       uint64_t bases_bytes, const uint64_t *h_off, BusyPair &busy) {
    const double t0 = PhaseTrace::now();
    int rc = parsed ? hulk::ctx_wait_event(R.ctx, parsed) : HULK_OK;
    if (rc == HULK_OK) rc = hulk::add_reads_device(R.ctx, d_bases, d_off, n, max_len, bases_bytes, h_off);
    if (rc == HULK_OK) rc = busy.mark(R.ctx);
    R.tr.add_reads += PhaseTrace::now() - t0;
    return rc == HULK_OK ? true : R.err.set(rc, hulk_last_error(R.ctx));
}

// The blocks given to the device whose results have not been taken, oldest first: `depth` of them stay queued behind the one
// whose result is due, and at the end of the stream the rest is due in order.  A run's loop:
//     while (<the parser goes on> && P.more()) {
//         if (P.next(it)) { <queue block P.b>; P.hold(it); }
//         if (!P.due()) continue;
//         <take the result of block P.oldest()>; P.release();
//     }
struct Pump {
    RawReader &reader; PhaseTrace &tr; IngestError &err; const size_t depth;
    std::deque<RawReader::Item> held;
    uint64_t b = 0;                                              // blocks queued so far (the next block's number)
    bool ended = false;                                          // the reader has nothing more (or has failed: err)
    double t_got = 0;
    Pump(RawReader &r, PhaseTrace &t, IngestError &e, size_t d) : reader(r), tr(t), err(e), depth(d) {}
    bool more() const { return err.code == HULK_OK && (!ended || !held.empty()); }
    bool next(RawReader::Item &it) {                             // the stream's next block, if there is one
        if (ended) return false;
        const double t0 = PhaseTrace::now();
        bool got = reader.next(it, err);
        t_got = PhaseTrace::now(); tr.wait_block += t_got - t0;
        if (got && it.len == 0) { reader.recycle(it.idx); got = false; }     // (end of the stream right on a block border)
        if (!got) ended = true;
        return got;
    }
    void hold(const RawReader::Item &it) {                       // its copy and kernels are queued
        tr.enqueue += PhaseTrace::now() - t_got;
        held.push_back(it); b++;
        if (it.eof) ended = true;
    }
    bool due() const { return err.code == HULK_OK && (held.size() > depth || (ended && !held.empty())); }
    uint64_t oldest() const { return b - held.size(); }
    void release() { reader.recycle(held.front().idx); held.pop_front(); }
};

// ------------------------------------------------------------------------------------------
// The device FASTQ run (the streams, buffers and their counts: at FqDev).
// ------------------------------------------------------------------------------------------
struct FqRun {
    DevRun &R; FqDev *D; IngestError &err;
    GpuSink sink;                                                // the host parser's way into the context, should it take over
    Parser hp;
    uint64_t n_lines = 0, dev_seqs = 0, dev_len = 0;
    uint32_t last_tail_lines = 0;
    bool on_host = false;                                        // the host parser has taken the stream over
    std::vector<uint8_t> carry;                                  // host take-over: bytes behind the last '\n' handed to the parser
    FqRun(DevRun &r) : R(r), D(r.D), err(r.err), sink(r.ctx, r.tr), hp(sink, r.cfg.parser_threads ? r.cfg.parser_threads : default_parser_threads(), r.err) {}

    // block b's copy and parse kernels
    bool queue_block(uint64_t b, const RawReader::Item &it) {
        const int r = (int)(b % FqDev::NRAW), o = (int)(b % FqDev::NOUT), st = (int)(b % FqDev::NST);
        // raw slot r held block b - NRAW and served block b - NRAW + 1 as the source of its tail
        if (!queue_copy(D, it, r, b >= (uint64_t)FqDev::NRAW ? D->ev_parsed[(b - FqDev::NRAW + 1) % FqDev::NST] : nullptr, err)) return false;
        // (the busy marks of the output sets survive between runs: the binning kernels of the run before — this context's or
        //  another's — may still be reading a set when this run's first parse is queued; its events say when they are done)
        ING_HIP(D->out_busy[o].wait(D->ps));
        ING_HIP(hulk::launch_fq_parse(D->ps, D->B, b ? D->d_raw[(b - 1) % FqDev::NRAW] : nullptr, b ? D->d_state + (b - 1) % FqDev::NST : nullptr,
                                      D->d_raw[r], D->d_state + st, (uint32_t)it.len, D->d_off[o], D->d_bases[o]));
        return state_back(D, D->h_state + st, D->d_state + st, sizeof(hulk::FqState), st, err);
    }
    // the reads of block x (parsed on the device) -> the context; false: failure (err) — or the host takes over (on_host)
    bool consume(uint64_t x) {
        const int st = (int)(x % FqDev::NST), o = (int)(x % FqDev::NOUT);
        const double tw0 = PhaseTrace::now();
        if (hipEventSynchronize(D->ev_parsed[st]) != hipSuccess) return err.set(HULK_ERR_HIP, "hipEventSynchronize (device FASTQ parser)");
        R.tr.stage_wait += PhaseTrace::now() - tw0;
        const hulk::FqState S = D->h_state[st];
        if (S.need_host) {
            // the stream goes to the host parser from the last record boundary: the previous block's tail (still in its raw
            // buffer on the device), then this block's bytes and everything behind it, out of the pinned buffers
            on_host = true;
            if (hipStreamSynchronize(D->ps) != hipSuccess) return err.set(HULK_ERR_HIP, "hipStreamSynchronize (device FASTQ parser)");
            carry.clear();
            if (x > 0) {
                const hulk::FqState Pv = D->h_state[(x - 1) % FqDev::NST];
                carry.resize(Pv.tail_len);
                if (Pv.tail_len && hipMemcpy(carry.data(), D->d_raw[(x - 1) % FqDev::NRAW] + Pv.tail_start, Pv.tail_len, hipMemcpyDeviceToHost) != hipSuccess)
                    return err.set(HULK_ERR_HIP, "hipMemcpy (tail of the device FASTQ parser)");
            }
            return true;
        }
        const uint64_t n = S.n_seq - S.pending;
        n_lines += S.n_lines - S.tail_lines; last_tail_lines = S.tail_lines;
        if (n == 0) return true;
        if (!check_read_lengths(S.min_len, S.max_len, R.min_len, err)) return false;
        if (!add_parsed(R, D->ev_parsed[st], D->d_bases[o], D->d_off[o], n, S.max_len, D->B.bytes_cap + 64, nullptr, D->out_busy[o])) return false;
        dev_seqs += n; dev_len += S.seq_bytes - S.pending_len;
        return true;
    }
    // the host parser over one raw block (cut anywhere): everything up to the last '\n', the rest is carried
    bool host_feed(const RawReader::Item &it) {
        if (!host_bytes(D, it, err)) return false;
        const uint8_t *p = D->h_buf[it.idx];
        carry.insert(carry.end(), p, p + it.len);
        size_t cut = carry.size();
        while (cut > 0 && carry[cut - 1] != '\n') cut--;
        const bool too_long = !it.eof && carry.size() - cut >= MAX_TOKEN;
        bool r = true;
        if (cut || too_long) r = hp.fastq_bytes(carry.data(), cut, too_long);
        carry.erase(carry.begin(), carry.begin() + cut);
        return r;
    }
    // after the take-over: the blocks the device had been given but whose reads were not handed over, in order, then the rest
    // of the stream
    bool host_rest(Pump &P) {
        bool ok = true, eof = false;
        while (ok && !P.held.empty()) {
            ok = host_feed(P.held.front()); eof = P.held.front().eof;
            P.release();
        }
        while (ok && !eof) {
            RawReader::Item it;
            if (!P.reader.next(it, err)) return err.code == HULK_OK;
            ok = host_feed(it); eof = it.eof;
            P.reader.recycle(it.idx);
        }
        return ok;
    }
};

// hulk_sketch_files over the device parser
static int run_ingest_device(hulk_ctx *ctx, const char *const *paths, uint32_t n_paths, const IngestCfg &cfg_in, PhaseTrace &g_trace,
                             hulk_ingest_stats *stats, IngestError &err) {
    DevRun R(ctx, g_trace, err);
    if (!R.begin(paths, n_paths, cfg_in, false)) return err.code;
    FqRun Q(R);
    {
        RawReader reader(paths, n_paths, R.cfg, R.D);
        Pump P(reader, g_trace, err, FqDev::DEPTH);
        while (!Q.on_host && P.more()) {
            RawReader::Item it;
            if (P.next(it)) { if (!Q.queue_block(P.b, it)) break; P.hold(it); }
            if (!P.due()) continue;                               // block b - DEPTH, while the blocks behind it are copied and parsed
            if (!Q.consume(P.oldest()) || Q.on_host) break;
            P.release();
        }
        bool ok = err.code == HULK_OK;
        if (ok && Q.on_host) ok = Q.host_rest(P);
        if (ok && !Q.on_host) Q.n_lines += Q.last_tail_lines;      // a record in progress at the end of the stream is dropped, its lines were read
        if (ok) ok = Q.sink.finish(err);
        R.end(reader, stats, Q.sink.n_seqs + Q.dev_seqs, Q.sink.total_len + Q.dev_len, Q.n_lines + Q.hp.n_lines);
    }
    if (R.cfg.trace)
        fprintf(stderr, "ingest trace (device FASTQ parser%s; calling thread, s): next block %.3f | copies + parse kernels queued %.3f, "
                        "waiting for a block's scalars %.3f, hulk_add_reads_device %.3f, host parser %.3f\n", Q.on_host ? ", host parser took over" : "",
                g_trace.wait_block, g_trace.enqueue, g_trace.stage_wait, g_trace.add_reads, g_trace.parse);
    return err.code;
}

// ------------------------------------------------------------------------------------------
// --fasta -> sequences ON THE DEVICE (hulk_fastq.hip, k_fa_*): sketch.go:102-135 with the host reduced to read() into pinned
// memory, one PCIe copy per block and the bookkeeping of records in stream order.  Unlike FASTQ a block's result depends on
// where the previous block left the accumulation buffer, and the host learns that from the previous block's scalars: the parse
// kernels of block b are queued when block b-1's scalars have arrived (its copy was queued before: the link stays busy, and
// the parse of a block is shorter than its copy).
//   acc[cur]     : [records handed over][complete records][record in progress]; rec_off[cur][r] = where record r begins
//   a batch      : the complete records, handed to hulk_add_reads_device when they hold FASTA_BATCH_BYTES (the host parser's
//                  rule) or the offsets run short; the record in progress then moves to the front of the other buffer
//   events       : an empty line ends the stream (sketch.go:103-105), a line of 64 KiB or more is bufio.Scanner's error — the
//                  first of the two in stream order counts, as in Parser::fasta_block
// ------------------------------------------------------------------------------------------
static bool fa_ensure(FqDev *D, IngestError &err) {
    FqDev::Fasta &F = D->fa;
    if (F.ready) return true;
    const uint32_t line_cap = (uint32_t)((MAX_TOKEN + D->block) / 2 + 2);
    const size_t nchunk = (D->raw_bytes() + 4095) / 4096 + 8, nlwg = ((size_t)line_cap + 255) / 256 + 8;     // (hulk_fastq.hip FA_T = 256)
    for (auto &B : F.B) {
        B.porch = D->porch; B.line_cap = line_cap;
        ING_HIP(hipMalloc((void **)&B.wgcnt, nchunk * 4));
        ING_HIP(hipMalloc((void **)&B.line_end, (size_t)line_cap * 4));
        ING_HIP(hipMalloc((void **)&B.linfo, (size_t)line_cap * 4));
        ING_HIP(hipMalloc((void **)&B.ldst, (size_t)line_cap * 4));
        ING_HIP(hipMalloc((void **)&B.hrel, (size_t)line_cap * 4));
        ING_HIP(hipMalloc((void **)&B.wghdr, nlwg * 4));
        ING_HIP(hipMalloc((void **)&B.wgbytes, nlwg * 8));
    }
    ING_HIP(hipMalloc((void **)&F.d_state, FqDev::NST * sizeof(hulk::FaState)));
    ING_HIP(hipHostMalloc((void **)&F.h_state, FqDev::NST * sizeof(hulk::FaState), hipHostMallocDefault));
    F.rec_cap = (size_t)line_cap + ((size_t)1 << 19);
    for (int i = 0; i < 2; i++) {
        F.acc_cap[i] = (size_t)192 << 20;
        ING_HIP(hipMalloc((void **)&F.acc[i], F.acc_cap[i] + 64));
        ING_HIP(hipMalloc((void **)&F.rec_off[i], (F.rec_cap + 2) * 8));
        for (auto &e : F.acc_busy[i].ev) ING_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    for (auto &e : F.ev_placed) ING_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ING_HIP(hipDeviceSynchronize());
    F.ready = true;
    return true;
}

struct FaRun {
    DevRun &R; FqDev *D; FqDev::Fasta &F; IngestError &err;
    // the stream's books
    int cur = 0;                     // the accumulation buffer the blocks are placed in
    uint64_t acc_len = 0;            // bytes in acc[cur]
    uint64_t open_start = 0;         // where the record in progress begins in acc[cur]
    uint64_t rec_count = 0;          // headers recorded in rec_off[cur] (the last one opened the record in progress)
    uint64_t batch_start = 0;        // rec_off[cur][0]: where the records not handed over yet begin
    bool have_hdr = false;           // the stream has had a header line (sequence lines in front of the first belong to no record)
    uint64_t bmin = ~0ull, bmax = 0; // shortest / longest of the complete records not handed over yet
    bool stopped = false;            // the empty line that ends the parsing has been placed
    uint64_t n_lines = 0, dev_seqs = 0, bytes_done = 0;
    hipEvent_t last_placed = nullptr;
    std::vector<uint64_t> h_rec;     // a batch's record offsets on the host, for the long-sequence path's descriptors
    FaRun(DevRun &r) : R(r), D(r.D), F(r.D->fa), err(r.err) {}

    // a buffer is written from acc_len on; what the context still reads of it (records handed over by the run before) lies below —
    // except in a buffer taken over EMPTY: wait for its readers first
    bool wait_readers(int b) {
        return F.acc_busy[b].wait(D->ps) == hipSuccess ? true : err.set(HULK_ERR_HIP, "hipStreamWaitEvent (FASTA buffers)");
    }
    // room for `need` bytes in acc[b] (contents up to `keep` survive)
    bool ensure_acc(int b, uint64_t need, uint64_t keep) {
        if (need <= F.acc_cap[b]) return true;
        size_t nc = F.acc_cap[b];
        while (nc < need) nc *= 2;
        uint8_t *q = nullptr;
        if (hipStreamSynchronize(D->ps) != hipSuccess || hipMalloc((void **)&q, nc + 64) != hipSuccess)
            return err.set(HULK_ERR_HIP, "hipMalloc (FASTA accumulation buffer)");
        if (keep && hipMemcpy(q, F.acc[b], keep, hipMemcpyDeviceToDevice) != hipSuccess) { hipFree(q); return err.set(HULK_ERR_HIP, "hipMemcpy (FASTA accumulation buffer)"); }
        // (what the context queued on the old buffer has to be through before it goes: hipFree waits for the device)
        hipFree(F.acc[b]);
        F.acc[b] = q; F.acc_cap[b] = nc; F.acc_busy[b].clear();
        return true;
    }
    // hand the complete records of acc[cur] to the context; final: the record in progress is complete too (end of the stream)
    bool hand_over(bool final) {
        uint64_t n = rec_count ? rec_count - 1 : 0;
        if (final && have_hdr) {
            const uint64_t L = acc_len - open_start;
            bmin = std::min(bmin, L); bmax = std::max(bmax, L);
            if (hipMemcpyAsync(F.rec_off[cur] + rec_count, &acc_len, 8, hipMemcpyHostToDevice, D->ps) != hipSuccess || hipStreamSynchronize(D->ps) != hipSuccess)
                return err.set(HULK_ERR_HIP, "hipMemcpyAsync (last FASTA record)");
            n++;
        }
        if (n) {
            if (!check_read_lengths(bmin, bmax, R.min_len, err)) return false;
            const double tc1 = PhaseTrace::now();
            // the records' offsets, for the long-sequence path's descriptors (the parse stream gets there long before the binning would)
            h_rec.resize(n + 1);
            if (hipMemcpyAsync(h_rec.data(), F.rec_off[cur], (n + 1) * 8, hipMemcpyDeviceToHost, D->ps) != hipSuccess || hipStreamSynchronize(D->ps) != hipSuccess)
                return err.set(HULK_ERR_HIP, "hipMemcpyAsync (FASTA record offsets)");
            R.tr.add_reads += PhaseTrace::now() - tc1;
            if (!add_parsed(R, last_placed, F.acc[cur], F.rec_off[cur], n, (uint32_t)bmax, F.acc_cap[cur] + 64, h_rec.data(), F.acc_busy[cur])) return false;
            dev_seqs += n; bytes_done += (final ? acc_len : open_start) - batch_start;
        }
        bmin = ~0ull; bmax = 0;
        return true;
    }
    // the record in progress moves to the front of the other buffer; the next blocks are placed there
    bool switch_buffers(uint64_t room) {
        const int nb = cur ^ 1;
        const uint64_t part = have_hdr ? acc_len - open_start : 0;
        if (!wait_readers(nb)) return false;                         // (records of `nb` handed over two batches ago: it is written from byte 0 now)
        if (!ensure_acc(nb, part + room + 64, 0)) return false;
        if (part && hipMemcpyAsync(F.acc[nb], F.acc[cur] + open_start, part, hipMemcpyDeviceToDevice, D->ps) != hipSuccess)
            return err.set(HULK_ERR_HIP, "hipMemcpyAsync (FASTA record in progress)");
        if (hipMemsetAsync(F.rec_off[nb], 0, 8, D->ps) != hipSuccess) return err.set(HULK_ERR_HIP, "hipMemsetAsync (FASTA record offsets)");
        cur = nb; acc_len = part; open_start = 0; batch_start = 0; rec_count = have_hdr ? 1 : 0;
        return true;
    }
    // block b's copy, and its index: neither needs to know where the blocks before left the accumulation buffer
    bool queue_block(uint64_t b, const RawReader::Item &it) {
        const int r = (int)(b % FqDev::NRAW), st = (int)(b % FqDev::NST);
        if (!queue_copy(D, it, r, b >= (uint64_t)FqDev::NRAW ? F.ev_placed[r] : nullptr, err)) return false;     // (behind the block that used this raw slot)
        ING_HIP(hulk::launch_fa_index(D->ps, F.B[b & 1], b ? D->d_raw[(b - 1) % FqDev::NRAW] : nullptr, b ? F.d_state + (b - 1) % FqDev::NST : nullptr,
                                      D->d_raw[r], F.d_state + st, (uint32_t)it.len));
        return state_back(D, F.h_state + st, F.d_state + st, sizeof(hulk::FaState), st, err);
    }
    // Block x has been indexed: its scalars -> the stream's books, its sequence lines -> the accumulation buffer.
    // false: the run fails (err).  Sets `stopped` at the empty line that ends the parsing.
    bool place(uint64_t x) {
        const int st = (int)(x % FqDev::NST), r = (int)(x % FqDev::NRAW);
        const double tw0 = PhaseTrace::now();
        if (hipEventSynchronize(D->ev_parsed[st]) != hipSuccess) return err.set(HULK_ERR_HIP, "hipEventSynchronize (device FASTA parser)");
        R.tr.stage_wait += PhaseTrace::now() - tw0;
        const hulk::FaState S = F.h_state[st];
        const bool stop = S.first_empty != hulk::FA_NONE && S.first_empty < S.long_line;
        const bool too_long = S.long_line != hulk::FA_NONE && !stop;
        n_lines += stop ? (uint64_t)S.first_empty + 1 : too_long ? (uint64_t)S.long_line : (uint64_t)S.n_lines;
        // as Parser::fasta_block: the first of the two events in stream order counts; a line too long ends the run with nothing handed over
        if (too_long) return err.set(HULK_ERR_LINE_TOO_LONG, hulk_strerror(HULK_ERR_LINE_TOO_LONG));
        // the offsets could not take this block's headers: a batch ends early
        if (rec_count + S.n_hdr + 2 > F.rec_cap && (!hand_over(false) || !switch_buffers(S.seq_bytes))) return false;
        if (!ensure_acc(cur, acc_len + S.seq_bytes + 64, acc_len)) return false;
        const double tq0 = PhaseTrace::now();
        if (S.seq_bytes || S.n_hdr) {
            const hipError_t e = hulk::launch_fa_place(D->ps, F.B[x & 1], D->d_raw[r], F.d_state + st, F.acc[cur], acc_len, F.rec_off[cur] + rec_count);
            if (e != hipSuccess) return err.set(HULK_ERR_HIP, std::string("launch_fa_place: ") + hipGetErrorString(e));
        }
        if (hipEventRecord(F.ev_placed[r], D->ps) != hipSuccess) return err.set(HULK_ERR_HIP, "hipEventRecord (FASTA block placed)");
        last_placed = F.ev_placed[r];
        R.tr.enqueue += PhaseTrace::now() - tq0;
        if (S.n_hdr) {
            const uint64_t first = acc_len + S.first_hdr, last = acc_len + S.last_hdr;
            if (have_hdr) { const uint64_t L = first - open_start; bmin = std::min(bmin, L); bmax = std::max(bmax, L); }
            else batch_start = first;                               // (sequence lines in front of the stream's first header: no record owns them)
            if (S.n_hdr > 1) { bmin = std::min<uint64_t>(bmin, S.min_len); bmax = std::max<uint64_t>(bmax, S.max_len); }
            rec_count += S.n_hdr; open_start = last; have_hdr = true;
        }
        acc_len += S.seq_bytes;
        if (!have_hdr) acc_len = 0;                                 // (l2 = nil: sequence lines before any header are dropped)
        if (stop) { stopped = true; return true; }
        if (S.tail_len >= MAX_TOKEN) return err.set(HULK_ERR_LINE_TOO_LONG, hulk_strerror(HULK_ERR_LINE_TOO_LONG));
        // a batch is due (the host parser's rule)
        if (rec_count > 1 && open_start - batch_start >= FASTA_BATCH_BYTES && (!hand_over(false) || !switch_buffers(0))) return false;
        return true;
    }
};

static int run_ingest_fasta_device(hulk_ctx *ctx, const char *const *paths, uint32_t n_paths, const IngestCfg &cfg_in, PhaseTrace &g_trace,
                                   hulk_ingest_stats *stats, IngestError &err) {
    DevRun R(ctx, g_trace, err);
    if (!R.begin(paths, n_paths, cfg_in, true)) return err.code;
    FaRun A(R);
    {
        RawReader reader(paths, n_paths, R.cfg, R.D);
        if (!A.wait_readers(0) || !A.wait_readers(1)) return err.code;
        Pump P(reader, g_trace, err, 1);                          // one block is placed while the next crosses the link and is indexed
        while (!A.stopped && P.more()) {
            RawReader::Item it;
            if (P.next(it)) { if (!A.queue_block(P.b, it)) break; P.hold(it); }
            if (!P.due()) continue;
            if (!A.place(P.oldest())) break;
            P.release();
        }
        if (err.code == HULK_OK) {
            // sketch.go:126-135 flushes the final entry unconditionally; with no header line at all the reference dies on l1[0] = 64
            if (!A.have_hdr) err.set(HULK_ERR_FASTA_HEADER, hulk_strerror(HULK_ERR_FASTA_HEADER));
            else A.hand_over(true);
        }
        R.end(reader, stats, A.dev_seqs, A.bytes_done, A.n_lines);
    }
    if (R.cfg.trace)
        fprintf(stderr, "ingest trace (device FASTA parser; calling thread, s): next block %.3f | copies + kernels queued %.3f, "
                        "waiting for a block's scalars %.3f, hulk_add_reads_device %.3f\n",
                g_trace.wait_block, g_trace.enqueue, g_trace.stage_wait, g_trace.add_reads);
    return err.code;
}

}  // namespace
}  // namespace ingest
}  // namespace hulk

using namespace hulk::ingest;

extern "C" {

int hulk_sketch_files_opts(hulk_ctx *ctx, const char *const *paths, uint32_t n_paths, int fasta, const hulk_ingest_opts *opts,
                           hulk_ingest_stats *stats) {
    if (!ctx) return HULK_ERR_ARG;
    if (const std::string bad = check_opts(opts); !bad.empty()) return hulk::ctx_fail(ctx, HULK_ERR_ARG, bad.c_str());
    IngestError err;
    int rc;
    {
        PhaseTrace trace;
        const IngestCfg cfg = resolve_cfg(opts, 0);
        if (!fasta && !cfg.host_parser) rc = run_ingest_device(ctx, paths, n_paths, cfg, trace, stats, err);
        else if (fasta && !cfg.host_parser) rc = run_ingest_fasta_device(ctx, paths, n_paths, cfg, trace, stats, err);
        else {
            GpuSink sink(ctx, trace);
            rc = run_ingest(paths, n_paths, fasta, cfg, sink, trace, stats, err);
        }
    }
    if (rc != HULK_OK) return hulk::ctx_fail(ctx, rc, err.msg.c_str());
    return HULK_OK;
}

int hulk_sketch_files(hulk_ctx *ctx, const char *const *paths, uint32_t n_paths, int fasta, uint32_t threads,
                      hulk_ingest_stats *stats) {
    hulk_ingest_opts o; memset(&o, 0, sizeof o);
    o.parser_threads = threads;
    return hulk_sketch_files_opts(ctx, paths, n_paths, fasta, threads ? &o : nullptr, stats);
}

}  // extern "C"
