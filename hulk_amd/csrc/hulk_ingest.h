// hulk_ingest.h — what the units of the host ingest share (private to libhulkhip.so):
//   hulk_ingest_gzip.hip    the gzip readers (one thread, BGZF members side by side, one member on several threads)
//   hulk_ingest_source.hip  the region pool, the byte source over the inputs, the block reader of the host parser
//   hulk_ingest_host.hip    the host parsers and hulk_parse_files: no context, no HIP runtime
//   hulk_ingest_device.hip  the sink into a context, the device parsers' run loops and hulk_sketch_files
// The first three link without the context and without the HIP runtime (tools/tsan_ingest.sh builds them alone).
#pragma once
#include <stdint.h>
#include <string.h>
#include <sys/types.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hulk_hip.h"

namespace hulk {
namespace bgzf { struct DevBufs; class DevReader; }
// (hidden: none of this is part of the library's dynamic symbol table)
namespace ingest __attribute__((visibility("hidden"))) {

constexpr size_t MAX_TOKEN = 64 * 1024;      // bufio.MaxScanTokenSize
// The knobs of ONE run (hulk_ingest_opts, include/hulk_hip.h): resolved once by run_ingest — defaults, then the caller's
// fields, then the HULK_* environment variables as overrides for profiling scripts and tests — and handed down to the
// readers; two runs side by side (two contexts of one host process) do not share them.
struct IngestCfg {
    size_t block = (size_t)(32u << 20);       // bytes per block of the line pump (>= 128 KiB)
    unsigned parser_threads = 0;              // 0: one per hardware thread, at most 16 (more were measured slower)
    unsigned gz_threads = 16;                 // members of a bgzip'd input / chunks of ONE gzip member inflated side by side
    bool gz_par = true;                       // one ordinary gzip member on gz_threads threads (GzPar)
    size_t gz_chunk = (size_t)(1u << 20);     // GzPar: compressed bytes per chunk (>= 8 KiB)
    unsigned readers = 4;                     // pieces a block of a regular file is pread() in, side by side
    bool zlib = false;                        // zlib's inflate instead of fast_inflate.h
    bool trace = false;                       // per-phase seconds on stderr
    bool host_parser = false;                 // FASTQ lines -> reads on the host's parser threads instead of the device
    bool dev_inflate = false;                 // the device parsers: bgzip'd files inflated on the GPU (hulk_bgzf.hip)
    bool block_set = false, readers_set = false;   // the caller (or the environment) chose; else the device path takes its own defaults
};
constexpr size_t FASTA_BATCH_BYTES = 64u << 20;

struct IngestError {
    int code = HULK_OK;
    std::string msg;
    bool set(int c, const std::string &m) { if (code == HULK_OK) { code = c; msg = m; } return false; }
};

// hulk_ingest_host.hip: a run's knobs from the caller's options and the environment; the caller's options checked
IngestCfg resolve_cfg(const hulk_ingest_opts *o, uint32_t threads);
std::string check_opts(const hulk_ingest_opts *o);
// IngestCfg::parser_threads == 0: one per hardware thread, at most 16 — 32 and 64 were measured slower on a 256-thread host
inline uint32_t default_parser_threads() {
    const uint32_t hw = std::thread::hardware_concurrency();
    return hw == 0 ? 1 : hw > 16 ? 16 : hw;
}

// A gzip'd input as a stream of text (hulk_ingest_gzip.hip).  The readers own the descriptor and close it.
struct GzStream {
    virtual ~GzStream() {}
    virtual long read(uint8_t *dst, size_t cap, std::string &msg) = 0;      // up to cap bytes; 0 = end of the stream; -1 = error (msg filled)
};
// the reader for the gzip file open at `fd` (its magic already checked): zlib's when the run asks for it (nullptr: zlib could not
// open the stream), else BGZF members side by side, one member on several threads, or the one-thread reader
std::unique_ptr<GzStream> gz_open(int fd, bool regular, const IngestCfg &cfg);
// the one-thread reader from the descriptor's position on; `first` = the stream starts here (an invalid first header is an error)
std::unique_ptr<GzStream> gz_open_sequential(int fd, bool first);

// Large scratch buffers of the gzip readers: anonymous mappings that ask for transparent huge pages (a first touch by 16+
// threads at once is otherwise 4 KiB page faults queueing on the process's mapping lock).  HULK_GZ_NO_THP=1: plain pages.
// Regions handed back are kept by the PROCESS for a while (RegionPool): the kernel zeroes pages when they are mapped and, on the
// GPU box, takes as long again to take them back — a run over one 100 MB FASTA file spent 10 ms faulting ~330 MB of block,
// piece and batch buffers in and 16 ms unmapping them, next to 10 ms of parsing (HULK_INGEST_TRACE).  A second file of the
// process finds the regions mapped and touched.  Bounded in size (POOL_BYTES) and in age (FQ_IDLE_SECONDS, swept with the device
// parser's sets: fq_sweep_idle; hulk_release_caches() unmaps at once).  Contents are NOT zeroed on reuse (no user relies on it).
struct RegionPool {
    struct Ent { void *p; size_t n; double t; };
    static constexpr size_t POOL_BYTES = (size_t)1 << 30, ONE_MAX = (size_t)256 << 20;
    std::mutex mu; std::vector<Ent> v; size_t bytes = 0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    static RegionPool &get() { static RegionPool *g = new RegionPool(); return *g; }      // (never destroyed: buffers of static objects may come back late)
    void *take(size_t n);                                   // a region of exactly n bytes (sizes are few: block, piece and batch buffers)
    bool give(void *p, size_t n);
    void sweep(double older_than);
};
struct BigBuf {
    void *p = nullptr; size_t n = 0;
    BigBuf() {}
    explicit BigBuf(size_t bytes) { reset(bytes); }
    BigBuf(const BigBuf &) = delete;
    BigBuf &operator=(const BigBuf &) = delete;
    ~BigBuf() { release(); }
    void release();
    void reset(size_t bytes);
    template <class T> T *as() const { return (T *)p; }
};
// ... with the few members of std::vector<uint8_t> the block reader uses (growing does NOT keep the contents)
struct PageBuf {
    BigBuf m; size_t sz = 0;
    uint8_t *data() const { return m.as<uint8_t>(); }
    size_t size() const { return sz; }
    void resize(size_t n) { if (n > m.n) m.reset(n); sz = n; }
    uint8_t &operator[](size_t i) const { return data()[i]; }
    uint8_t *begin() const { return data(); }
};

// ------------------------------------------------------------------------------------------
// A team of workers that stay around.  run(n, f) calls f(0) .. f(n-1), each once, on the caller and the workers, and returns
// when all are done.  Every parallel step of the ingest path was a fork-join of freshly created threads (two per 32 MB block
// in the parser, three per batch in the gzip readers, one per large copy): hundreds of creations per second of run, each a
// stack mapping under the process's mapping lock, at the moment when dozens of other threads take page faults under the same
// lock.  Indices are handed out one at a time (a task may wait for a LATER index's early result — GzPar's chunks do —, never
// for an earlier one's: the lowest running task can always finish, so fewer awake threads than tasks cannot deadlock).
// ------------------------------------------------------------------------------------------
class Team {
 public:
    explicit Team(unsigned workers) { for (unsigned i = 0; i < workers; i++) th_.emplace_back([this] { loop(); }); }
    ~Team() {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    unsigned size() const { return (unsigned)th_.size() + 1; }
    template <class F> void run(unsigned n, F &&f) {
        if (n <= 1 || th_.empty()) { for (unsigned i = 0; i < n; i++) f(i); return; }
        const std::function<void(unsigned)> job(std::ref(f));
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = &job; n_ = n; next_.store(0, std::memory_order_relaxed); pending_ = (unsigned)th_.size(); gen_++;
        }
        cv_.notify_all();
        std::exception_ptr mine;                         // the caller's own share may throw too: the workers still hold `job`
        try {
            for (unsigned i; (i = next_.fetch_add(1, std::memory_order_relaxed)) < n;) f(i);
        } catch (...) {
            mine = std::current_exception();
            next_.store(n, std::memory_order_relaxed);   // nothing more is handed out
        }
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return pending_ == 0; });   // ... and nobody touches `job` or the caller's buffers after this
        if (mine) { failed_ = nullptr; std::rethrow_exception(mine); }
        if (failed_) { std::exception_ptr e = failed_; failed_ = nullptr; std::rethrow_exception(e); }
    }

 private:
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> g(m_);
            cv_.wait(g, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            const std::function<void(unsigned)> *job = job_; const unsigned n = n_;
            g.unlock();
            try {
                for (unsigned i; (i = next_.fetch_add(1, std::memory_order_relaxed)) < n;) (*job)(i);
            } catch (...) {                                 // a worker has no caller to unwind to: run() rethrows it in the caller's thread
                next_.store(n, std::memory_order_relaxed);
                g.lock();
                if (!failed_) failed_ = std::current_exception();
                g.unlock();
            }
            g.lock();
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    uint64_t gen_ = 0; bool stop_ = false;
    const std::function<void(unsigned)> *job_ = nullptr; unsigned n_ = 0, pending_ = 0;
    std::atomic<unsigned> next_{0};
    std::exception_ptr failed_;
};

// ------------------------------------------------------------------------------------------
// Sequential byte source over the inputs.  bufio.Scanner is per input: an unterminated last line is
// a token of THAT input, so a '\n' is supplied at the end of an input that does not end in one.
// ------------------------------------------------------------------------------------------
class ByteSource {
 public:
    ByteSource(const char *const *paths, uint32_t n, const IngestCfg &cfg);
    ~ByteSource();
    // HULK_INGEST_DEVICE_INFLATE: a regular file whose first member is BGZF is inflated on the device (hulk_bgzf.hip); its
    // text is then delivered to device memory (read's `ddst`) instead of `dst`
    void set_device_inflate(hulk::bgzf::DevBufs *b) { dev_bufs_ = b; }

    // up to cap bytes into dst; 0 = all inputs exhausted; -1 = error.  With `ddst` (device memory for up to cap bytes), bytes that
    // are device text go there and *on_dev says so.
    long read(uint8_t *dst, size_t cap, IngestError &err, uint8_t *ddst = nullptr, bool *on_dev = nullptr);

 private:
    IngestCfg cfg_;                                          // this run's knobs (resolve_cfg)
    // A single read() out of the page cache is one core's memcpy (~10 GB/s), slower than the parser behind
    // it: large requests on a regular file are cut into pieces that are pread() side by side.
    static constexpr size_t PAR_READ_MIN = 8u << 20;
    unsigned readers() const { return cfg_.readers; }
    long read_pieces(uint8_t *dst, size_t cap);
    std::string current_name() const { return stdin_mode_ ? "STDIN" : paths_[idx_]; }
    bool open_path(const std::string &p, IngestError &err);
    void close_current();
    std::vector<std::string> paths_;
    size_t idx_ = 0;
    bool stdin_mode_ = false, stdin_done_ = false, open_ = false, got_any_ = false;
    int fd_ = -1;
    bool regular_ = false;
    off_t pos_ = 0;
    std::unique_ptr<GzStream> gzf_;
    hulk::bgzf::DevBufs *dev_bufs_ = nullptr;
    std::unique_ptr<hulk::bgzf::DevReader> dgz_;
    uint8_t last_ = '\n';
    std::unique_ptr<Team> team_;                                  // read_pieces' readers
};

// ------------------------------------------------------------------------------------------
// Reader thread: blocks that end on '\n' (the unterminated tail is carried into the next block).
// ------------------------------------------------------------------------------------------
struct Block {
    PageBuf buf;
    size_t len = 0;
    bool tail_too_long = false;   // the line after this block's last '\n' already has >= MAX_TOKEN bytes
};
class BlockReader {
 public:
    BlockReader(const char *const *paths, uint32_t n, const IngestCfg &cfg);
    ~BlockReader();
    // next block, or nullptr at the end / on error (err filled)
    std::unique_ptr<Block> next(IngestError &err);
    void recycle(std::unique_ptr<Block> b);
    uint64_t bytes_in() const { return bytes_in_; }

 private:
    void run();
    void finish(const IngestError &e);
    const size_t block_;                                     // IngestCfg::block
    ByteSource src_;
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::unique_ptr<Block>> q_, pool_;
    bool done_ = false, stop_ = false;
    IngestError err_;
    std::atomic<uint64_t> bytes_in_{0};                            // (read by the calling thread for the statistics, also while the reader still runs: an error stops the parser first)
};

// ------------------------------------------------------------------------------------------
// Sinks: where parsed sequences go.  prepare() hands out room for n sequences / nbytes bases
// (lens[i] receives the length of sequence i); commit() takes the first n_commit of them.
// ------------------------------------------------------------------------------------------
struct Sink {
    virtual ~Sink() {}
    virtual bool prepare(uint64_t n, uint64_t nbytes, uint8_t **bases, uint64_t **lens, IngestError &err) = 0;
    virtual bool commit(uint64_t n_commit, IngestError &err) = 0;     // lens -> offsets happens here
    virtual bool finish(IngestError &err) { (void)err; return true; }
    uint64_t n_seqs = 0, total_len = 0;
};

// lens[0..n) -> exclusive offsets in place (array has n+1 entries); returns total, min, max
inline uint64_t lens_to_offsets(uint64_t *a, uint64_t n, uint64_t &mn, uint64_t &mx) {
    uint64_t run = 0; mn = ~0ull; mx = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t L = a[i];
        if (L < mn) mn = L;
        if (L > mx) mx = L;
        a[i] = run; run += L;
    }
    a[n] = run;
    return run;
}

// a failed HIP call ends the function it stands in with `false` and the call's text in `err` (the units that use the HIP runtime)
#define ING_HIP(call)                                                                               \
    do { hipError_t e_ = (call); if (e_ != hipSuccess) return err.set(HULK_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

// HULK_INGEST_TRACE=1: seconds the calling thread spent in each phase of a run, on stderr when the run ends (diagnosis)
struct PhaseTrace {
    double wait_block = 0, parse = 0, stage_wait = 0, enqueue = 0, add_reads = 0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
};

// NewMinimizerSketch's checks (minimizer.go:70-76), as hulk_add_reads makes them: mn / mx = the shortest / longest sequence of
// a batch that goes to the context, min_len = the context's w + k - 1
inline bool check_read_lengths(uint64_t mn, uint64_t mx, uint64_t min_len, IngestError &err) {
    if (mn < 1) return err.set(HULK_ERR_EMPTY_SEQ, hulk_strerror(HULK_ERR_EMPTY_SEQ));
    if (mn < min_len) return err.set(HULK_ERR_SHORT_SEQ, hulk_strerror(HULK_ERR_SHORT_SEQ));
    if (mx > 0xffffffffull) return err.set(HULK_ERR_READ_TOO_LONG, hulk_strerror(HULK_ERR_READ_TOO_LONG));
    return true;
}

// The host parsers (hulk_ingest_host.hip): blocks of whole lines -> sequences -> the sink.  The per-line loops are that unit's own.
struct Parser {
    Sink &sink; uint32_t threads; IngestError &err;
    uint64_t n_lines = 0;
    Parser(Sink &s, uint32_t t, IngestError &e) : sink(s), threads(t ? t : 1), err(e) {}

    // ---- FASTQ ----
    uint8_t fq_state = 0;
    std::vector<uint8_t> pending;      // sequence of the record in progress (l2 set, l4 not yet seen)
    bool have_pending = false;
    bool carry_bad = false; std::string carry_hdr;

    bool fastq_block(const Block &blk) { return fastq_bytes(blk.buf.data(), blk.len, blk.tail_too_long); }
    // `len` bytes that end in '\n'; tail_too_long: the unterminated line behind them already has MAX_TOKEN bytes
    bool fastq_bytes(const uint8_t *base, size_t blen, bool tail_too_long);
    bool bad_id(const std::string &hdr);

    // ---- FASTA ----
    struct RawBuf {                                                     // bytes without a constructor (a vector's resize zero-fills), on huge pages:
        uint8_t *p = nullptr; size_t n = 0, cap = 0;                    // 100 MB of 4 KB pages are 25 k page faults to fill and as many to unmap
        static constexpr size_t FIRST = (size_t)128 << 20;              // a batch (64 MB) + a block + a record's tail fit: growing is the exception,
        ~RawBuf();                                                      // and the region goes back to the process's pool
        uint8_t *grow(size_t add);
        void erase_front(size_t k) { if (k) { memmove(p, p + k, n - k); n -= k; } }
        size_t size() const { return n; }
    };
    struct FaPiece {
        std::unique_ptr<BigBuf> buf; size_t cap = 0, nbytes = 0;        // the piece's sequence bytes (huge pages; the buffer lives as long as the parser: no page faults per block)
        std::vector<uint64_t> hdr_at;                                   // offsets into buf at which a header line stood
        uint64_t n_lines = 0; bool stopped = false, too_long = false;   // lines seen up to the event; an empty line / a line of >= 64 KiB ends the piece
    };
    bool fa_have_hdr = false, fa_stopped = false;
    std::vector<FaPiece> fa_pieces;
    RawBuf fa_bases; std::vector<uint64_t> fa_lens; uint64_t fa_cur = 0;   // complete records (fa_lens) then the record in progress (fa_cur bytes)

    bool fasta_flush_batch(bool final_record);
    bool fasta_block(const Block &blk);
    bool fasta_end();

    template <class F> void run_parallel(uint32_t P, F f);             // (defined in, and used by, hulk_ingest_host.hip only)
    std::unique_ptr<Team> team_;
};

// hulk_parse_files, and hulk_sketch_files with HULK_INGEST_HOST_PARSER: the host's line pump over the inputs into `sink`
int run_ingest(const char *const *paths, uint32_t n_paths, int fasta, const IngestCfg &cfg, Sink &sink, PhaseTrace &g_trace,
               hulk_ingest_stats *stats, IngestError &err);

}  // namespace ingest
}  // namespace hulk
