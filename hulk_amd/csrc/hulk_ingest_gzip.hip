// The gzip readers of the host ingest (hulk_ingest.h): GzFast — one inflate thread, every kind of member, the exact errors and
// messages —, GzBgzf — the members of a bgzip'd file side by side — and GzPar — one ordinary member on several threads.  Neither
// the context nor the HIP runtime is used here.
#include <errno.h>
#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>

#include "hulk_ingest.h"
#include "fast_inflate.h"
#include "par_inflate.h"
#include "crc32_clmul.h"
#include "hulk_bgzf.h"

namespace hulk {
namespace ingest {
namespace {

// ------------------------------------------------------------------------------------------
// gzip reader on hulk::inflate (fast_inflate.h).  A producer thread inflates into 1 MB chunks (each
// with the previous chunk's last 32 KiB in front of it as match history); the consumer — the block
// reader's thread — takes the CRC-32 of a chunk (crc32_clmul.h) while copying it out, so that inflate
// and checksum run side by side.  Members are concatenated (compress/gzip's multistream default);
// what follows the last member and is not a gzip header is ignored, as zlib's gzread does.
// HULK_GZ_ZLIB=1 keeps zlib's inflate (gzread) instead.
// ------------------------------------------------------------------------------------------
class GzZlib : public GzStream {
 public:
    explicit GzZlib(gzFile gz) : gz_(gz) { gzbuffer(gz_, 1u << 20); }
    ~GzZlib() override { gzclose(gz_); }                          // gzclose closes the descriptor
    long read(uint8_t *dst, size_t cap, std::string &msg) override {
        const long n = gzread(gz_, dst, (unsigned)std::min<size_t>(cap, 1u << 30));
        if (n < 0) { int e = 0; const char *m = gzerror(gz_, &e); msg = std::string("gzip: ") + (m ? m : "read error"); }
        return n < 0 ? -1 : n;
    }

 private:
    gzFile gz_;
};

// where a reader that inflated the front of a member by other means (GzPar) hands the member over: the descriptor is positioned
// at the byte that holds the first bit of a block header, `bit` of its bits belong to the block in front; the last <= 32 KiB
// of text, and the CRC-32 / length of all the member's text so far
struct GzResume { int bit = 0; std::vector<uint8_t> hist; uint32_t crc = 0, size = 0; };

class GzFast : public GzStream {
 public:
    // `first` = the stream starts here (an invalid first header is an error; after a member it is the clean end)
    explicit GzFast(int fd, bool first = true, const GzResume *resume = nullptr) : fd_(fd), first_(first) {
        for (auto &c : chunks_) { c.buf.resize(HIST + CHUNK + hulk::inflate::OUT_SLACK + 64); free_.push_back(&c); }
        if (resume) { resume_ = *resume; resuming_ = true; crc_ = resume->crc; size_ = resume->size; }
        th_ = std::thread([this] { produce(); });
    }
    ~GzFast() {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        cv_.notify_all();
        if (th_.joinable()) th_.join();
        if (fd_ > 0) ::close(fd_);
    }
    // up to cap bytes; 0 = end of the stream; -1 = error (msg filled)
    long read(uint8_t *dst, size_t cap, std::string &msg) override {
        for (;;) {
            if (!cur_) {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [this] { return !ready_.empty(); });
                cur_ = ready_.front(); ready_.pop_front();
            }
            if (cur_->off < cur_->len) {
                const size_t n = std::min(cap, cur_->len - cur_->off);
                const uint8_t *src = cur_->buf.data() + HIST + cur_->off;
                // (zlib's crc32 takes a uInt length)
                crc_ = hulk::crc32_fast(crc_, src, n);
                memcpy(dst, src, n);
                cur_->off += n; size_ += (uint32_t)n;
                return (long)n;
            }
            // chunk drained: its end-of-member / end-of-stream / error marks
            if (cur_->member_end) {
                if (crc_ != cur_->crc || size_ != cur_->isize) { msg = "gzip: invalid checksum"; return -1; }
                crc_ = 0; size_ = 0;
            }
            if (!cur_->err.empty()) { msg = cur_->err; return -1; }
            const bool eof = cur_->eof;
            if (eof) return 0;                                     // (the chunk stays current: every later call ends here too)
            { std::lock_guard<std::mutex> g(m_); free_.push_back(cur_); }
            cv_.notify_all();
            cur_ = nullptr;
        }
    }

 private:
    static constexpr size_t HIST = 32768, CHUNK = 1u << 20, INBUF = 1u << 20;
    struct Chunk { std::vector<uint8_t> buf; size_t len = 0, off = 0; bool member_end = false, eof = false; uint32_t crc = 0, isize = 0; std::string err; };

    Chunk *get_free() {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [this] { return !free_.empty() || stop_; });
        if (stop_) return nullptr;
        Chunk *c = free_.back(); free_.pop_back();
        c->len = c->off = 0; c->member_end = c->eof = false; c->err.clear();
        return c;
    }
    void publish(Chunk *c) { { std::lock_guard<std::mutex> g(m_); ready_.push_back(c); } cv_.notify_all(); }

    // compressed input: inbuf_[ipos .. iend) is unread (the decoder's `in` pointer is the read position)
    bool refill() {                                                // keeps the unread tail; false = no more input
        const size_t tail = dec_.in ? dec_.in_left() : 0;
        if (tail) memmove(inbuf_.data(), dec_.in, tail);
        size_t got = 0;
        while (!in_eof_ && tail + got < INBUF) {
            const ssize_t m = ::read(fd_, inbuf_.data() + tail + got, INBUF - tail - got);
            if (m < 0) { if (errno == EINTR) continue; io_err_ = std::string("read: ") + strerror(errno); in_eof_ = true; break; }
            if (m == 0) { in_eof_ = true; break; }
            got += (size_t)m;
            break;                                                  // one read per refill is enough
        }
        memset(inbuf_.data() + tail + got, 0, 16);                  // the fast loop loads 8 bytes at a time
        dec_.feed(inbuf_.data(), tail + got);
        return got != 0;
    }
    bool next_byte(uint8_t &b) { while (!dec_.take_byte(b)) { if (!refill()) return false; } return true; }

    // 1 = header read, 0 = clean end (no more members), -1 = error (msg)
    int read_header(bool first, std::string &msg) {
        uint8_t h[10];
        for (int i = 0; i < 10; i++) {
            if (!next_byte(h[i])) {
                if (i == 0 && !first) return 0;
                if (!first && i < 2) return 0;                      // trailing bytes that are not a member
                msg = first && i == 0 ? "EOF" : "unexpected EOF"; return -1;
            }
            if (i == 1 && (h[0] != 0x1f || h[1] != 0x8b)) { if (!first) return 0; msg = "gzip: invalid header"; return -1; }
        }
        if (h[2] != 8) { msg = "gzip: invalid header"; return -1; }
        const uint8_t flg = h[3];
        uint8_t b;
        if (flg & 4) {                                              // FEXTRA
            uint8_t l0, l1; if (!next_byte(l0) || !next_byte(l1)) { msg = "unexpected EOF"; return -1; }
            for (uint32_t n = (uint32_t)l0 | ((uint32_t)l1 << 8); n; n--) if (!next_byte(b)) { msg = "unexpected EOF"; return -1; }
        }
        if (flg & 8) do { if (!next_byte(b)) { msg = "unexpected EOF"; return -1; } } while (b);     // FNAME
        if (flg & 16) do { if (!next_byte(b)) { msg = "unexpected EOF"; return -1; } } while (b);    // FCOMMENT
        if (flg & 2) { if (!next_byte(b) || !next_byte(b)) { msg = "unexpected EOF"; return -1; } }  // FHCRC (not verified)
        return 1;
    }

    // A member always starts a chunk (the end of a member ends its chunk), so the window of the running member is
    // the `hist_have` bytes in front of the chunk's data plus what the chunk holds so far.
    void produce() {
        inbuf_.resize(INBUF + 64);
        dec_.feed(inbuf_.data(), 0);
        Chunk *c = get_free();
        if (!c) return;
        auto finish = [&](Chunk *ch, size_t len, const std::string &e) { ch->len = len; ch->err = e; ch->eof = true; publish(ch); };
        bool first = first_;
        for (;;) {
            uint8_t *base = c->buf.data() + HIST, *out = base;
            size_t hist_have = 0;
            std::string msg;
            if (resuming_) {
                // in the middle of a member: no header; the reader starts `bit` bits into the first byte, the window is handed in
                resuming_ = false; first = false;
                dec_.reset();
                refill();
                dec_.refill_slow();
                if (dec_.bitcnt < resume_.bit) { finish(c, 0, !io_err_.empty() ? io_err_ : std::string("unexpected EOF")); return; }
                dec_.bitbuf >>= resume_.bit; dec_.bitcnt -= resume_.bit;
                hist_have = std::min(HIST, resume_.hist.size());
                memcpy(base - hist_have, resume_.hist.data() + resume_.hist.size() - hist_have, hist_have);
            } else {
                const int hr = read_header(first, msg);
                if (hr <= 0) { finish(c, 0, hr < 0 ? msg : io_err_); return; }
                first = false;
                dec_.reset();
            }
            for (;;) {
                uint8_t *lim = base + CHUNK;
                out = dec_.run(out, lim, base - hist_have, false);
                if (dec_.state == hulk::inflate::Decoder::DONE) break;
                if (dec_.state == hulk::inflate::Decoder::ERROR) { finish(c, (size_t)(out - base), std::string("gzip: ") + dec_.err); return; }
                if (out >= lim) {                                   // chunk full: hand it over, go on in the next one
                    c->len = (size_t)(out - base);
                    Chunk *nx = get_free();
                    if (!nx) return;
                    const size_t hh = std::min(HIST, hist_have + c->len);      // history = tail of (old history + chunk)
                    memcpy(nx->buf.data() + HIST - hh, out - hh, hh);
                    hist_have = hh;
                    publish(c); c = nx;
                    base = c->buf.data() + HIST; out = base;
                    continue;
                }
                if (!refill()) {                                    // starved and nothing more to read
                    out = dec_.run(out, lim, base - hist_have, true);          // reports the truncation
                    if (dec_.state == hulk::inflate::Decoder::DONE) break;
                    if (out >= lim) continue;
                    finish(c, (size_t)(out - base), !io_err_.empty() ? io_err_ : std::string("unexpected EOF"));
                    return;
                }
            }
            // trailer: CRC-32 and ISIZE, little endian, after the next byte boundary
            dec_.align_to_byte();
            uint8_t t[8];
            for (int i = 0; i < 8; i++) if (!next_byte(t[i])) { finish(c, (size_t)(out - base), "unexpected EOF"); return; }
            c->len = (size_t)(out - base);
            c->member_end = true;
            c->crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
            c->isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
            Chunk *nx = get_free();
            if (!nx) return;
            publish(c); c = nx;
        }
    }

    int fd_;
    bool first_;
    GzResume resume_;
    bool resuming_ = false;
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    Chunk chunks_[4];
    std::deque<Chunk *> free_, ready_;
    bool stop_ = false;
    // producer side
    hulk::inflate::Decoder dec_;
    std::vector<uint8_t> inbuf_;
    bool in_eof_ = false;
    std::string io_err_;
    // consumer side
    Chunk *cur_ = nullptr;
    uint32_t crc_ = 0, size_ = 0;
};

// One core copies ~8 GB/s out of a buffer another core wrote, less than several inflate threads deliver: large pieces are
// copied by four threads.  (Pieces of ceil(n / 4) rounded up to 64 bytes: with floor(n / 4), as first written, the last
// n mod 4 bytes were not copied whenever floor(n / 4) happened to be a multiple of 64.)
static void copy_wide(uint8_t *dst, const uint8_t *src, size_t n) {
    if (n < (8u << 20)) { memcpy(dst, src, n); return; }
    const unsigned R = 4;
    const size_t piece = ((n + R - 1) / R + 63) & ~(size_t)63;
    static thread_local Team team(R - 1);                      // (the block reader's thread is the only caller; gone with it)
    team.run(R, [&](unsigned i) { const size_t at = (size_t)i * piece; if (at < n) memcpy(dst + at, src + at, std::min(piece, n - at)); });
}

// ------------------------------------------------------------------------------------------
// BGZF (bgzip / htslib): a gzip file of members of <= 64 KiB of text whose headers carry the member's compressed size in a
// "BC" extra subfield — members are found without inflating and inflated SIDE BY SIDE (one inflate thread is what bounds a
// `.gz` run: 1.2-1.5 GB/s of text).  Purely an optimisation of the same stream semantics: a batch of members is located from
// the BSIZE fields, every member inflated into its own slice of the batch's output (size from its ISIZE trailer) and
// checked — stream ends exactly at the trailer, ISIZE bytes produced, CRC-32 equal.  At the first member that is anything
// else (no BC subfield, other header flags, truncated, any check failing) the members before it are delivered and the
// sequential reader (GzFast) takes the descriptor over from that member's offset: errors, trailing bytes and ordinary
// members keep the exact behaviour and messages of the one-thread path.  Regular files only (needs pread / lseek).
// HULK_GZ_THREADS (default 16, at most the hardware threads; 1 = off).
// ------------------------------------------------------------------------------------------
class GzBgzf : public GzStream {
 public:
    unsigned threads() const { return cfg_.gz_threads; }
    // total size of the member whose header starts at p (n bytes available), 0 = not a BGZF member / header incomplete
    static size_t member_size(const uint8_t *p, size_t n, size_t *header_len) { return hulk::bgzf::member_size(p, n, header_len); }
    static bool looks_like(int fd) {
        uint8_t h[64];
        const ssize_t m = ::pread(fd, h, sizeof h, 0);
        size_t hl;
        return m >= 18 && member_size(h, (size_t)m, &hl) != 0;
    }
    GzBgzf(int fd, const IngestCfg &cfg) : cfg_(cfg), fd_(fd) { th_ = std::thread([this] { produce(); }); }
    ~GzBgzf() override {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        cv_.notify_all();
        if (th_.joinable()) th_.join();
        if (cfg_.trace)
            fprintf(stderr, "ingest trace: BGZF reader, %llu members inflated by %u threads%s\n", (unsigned long long)n_members_,
                    threads(), tail_ ? ", then handed over to the sequential reader" : "");
        if (tail_) tail_.reset();                                  // (owns and closes the descriptor from then on)
        else if (fd_ > 0) ::close(fd_);
    }
    long read(uint8_t *dst, size_t cap, std::string &msg) override {
        for (;;) {
            if (tail_) return tail_->read(dst, cap, msg);
            if (!cur_) {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [this] { return !ready_.empty(); });
                cur_ = ready_.front(); ready_.pop_front();
            }
            if (cur_->off < cur_->out_len) {
                const size_t n = std::min(cap, cur_->out_len - cur_->off);
                const uint8_t *src = cur_->out.data() + cur_->off;
                copy_wide(dst, src, n);
                cur_->off += n;
                return (long)n;
            }
            if (!cur_->err.empty()) { msg = cur_->err; return -1; }
            if (cur_->hand_over >= 0) {                            // the rest of the file is the sequential reader's
                if (::lseek(fd_, cur_->hand_over, SEEK_SET) < 0) { msg = std::string("lseek: ") + strerror(errno); return -1; }
                tail_.reset(new GzFast(fd_, !cur_->any_member));
                continue;
            }
            if (cur_->eof) return 0;
            { std::lock_guard<std::mutex> g(m_); free_.push_back(cur_); }
            cv_.notify_all();
            cur_ = nullptr;
        }
    }

 private:
    IngestCfg cfg_;                                          // this run's knobs (resolve_cfg)
    static constexpr size_t IN_BATCH = 8u << 20;
    using Member = hulk::bgzf::Member;
    struct Batch {
        PageBuf in, out; std::vector<Member> mem;      // (huge-page mappings, not zero-filled by one thread: 16 inflate threads touch them first)
        size_t out_len = 0, off = 0; off_t hand_over = -1; bool eof = false, any_member = false; std::string err;
    };
    Batch *get_free() {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [this] { return !free_.empty() || stop_; });
        if (stop_) return nullptr;
        Batch *b = free_.back(); free_.pop_back();
        b->out_len = b->off = 0; b->hand_over = -1; b->eof = false; b->err.clear(); b->mem.clear();
        return b;
    }
    void publish(Batch *b) { { std::lock_guard<std::mutex> g(m_); ready_.push_back(b); } cv_.notify_all(); }
    // one member into its slice; false = anything at all is off (the sequential reader will say what)
    static bool inflate_member(const Batch &b, const Member &m, uint8_t *out) {
        hulk::inflate::Decoder d;
        d.feed(b.in.data() + m.in_off, m.in_len);
        uint8_t *base = out + m.out_off, *end = base + m.isize;
        // one byte of room beyond the slice: the end-of-block code is only read while there is room (a stream that
        // uses it is wrong and is caught by the position check; the byte belongs to a LATER member, which is dropped with it)
        uint8_t *o = d.run(base, end + 1, base, true);
        if (d.state != hulk::inflate::Decoder::DONE || o != end) return false;
        d.align_to_byte();
        if (d.in_left() + (size_t)(d.bitcnt >> 3) != 0) return false;           // the deflate stream ends where BSIZE says
        return hulk::crc32_fast(0, base, m.isize) == m.crc;
    }
    void produce() {
        off_t pos = 0;
        bool any = false;
        for (;;) {
            Batch *b = get_free();
            if (!b) return;
            b->any_member = any;
            b->in.resize(IN_BATCH);
            size_t got = 0;
            while (got < IN_BATCH) {
                const ssize_t r = ::pread(fd_, b->in.data() + got, IN_BATCH - got, pos + (off_t)got);
                if (r < 0) { if (errno == EINTR) continue; b->err = std::string("read: ") + strerror(errno); publish(b); return; }
                if (r == 0) break;
                got += (size_t)r;
            }
            if (got == 0) { b->eof = true; publish(b); return; }
            // the members that lie in this piece of the file, whole
            size_t out_total = 0;
            const size_t o = hulk::bgzf::frame(b->in.data(), got, b->mem, SIZE_MAX, SIZE_MAX, &out_total);
            // (a member cut by the end of the piece starts the next piece; one cut by the end of the FILE, or not a BGZF member, is
            // then the first thing of a piece: the sequential reader's from there on)
            if (b->mem.empty()) { b->hand_over = pos; publish(b); return; }
            if (b->out.size() < out_total + 1) b->out.resize(out_total + out_total / 16 + 1);
            const unsigned T = std::min<unsigned>(threads(), (unsigned)b->mem.size());
            std::atomic<size_t> next{0}, first_bad{b->mem.size()};
            auto work = [&]() {
                for (;;) {
                    const size_t j = next.fetch_add(1);
                    if (j >= b->mem.size() || j > first_bad.load()) return;
                    if (!inflate_member(*b, b->mem[j], b->out.data())) {
                        size_t cur = first_bad.load();
                        while (j < cur && !first_bad.compare_exchange_weak(cur, j)) {}
                    }
                }
            };
            if (!team_) team_.reset(new Team(threads() - 1));
            team_->run(T, [&](unsigned) { work(); });
            const size_t bad = first_bad.load();
            if (bad < b->mem.size()) {
                // everything in front of the first member that failed a check is good; that member starts the hand-over
                const Member &mb = b->mem[bad];
                b->out_len = mb.out_off;
                b->hand_over = pos + (off_t)mb.hdr_off;
                if (bad > 0) any = true;
                n_members_ += bad;
                b->any_member = any;
                publish(b);
                return;
            }
            b->out_len = out_total;
            any = true;
            pos += (off_t)o;
            n_members_ += b->mem.size();
            publish(b);
        }
    }

    int fd_;
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    Batch batches_[2];
    std::deque<Batch *> free_{&batches_[0], &batches_[1]}, ready_;
    bool stop_ = false;
    Batch *cur_ = nullptr;
    std::unique_ptr<GzFast> tail_;
    uint64_t n_members_ = 0;
    std::unique_ptr<Team> team_;                                  // the producer's
};

// ------------------------------------------------------------------------------------------
// ONE gzip member inflated by several threads (par_inflate.h has the how and why).  The compressed file is taken in batches
// of T chunks of 1 MB; a batch starts at a block boundary `q` that is known to the bit, with the 32 KiB of text in front of it.
// Chunk 0 decodes from q with that window; chunk j > 0 looks for a block header behind byte j MB and decodes from there into
// symbols, not knowing its window; every chunk runs until the first block boundary at or behind the start its successor
// found.  Chunk j's work COUNTS only if chunk j-1 counted and ended, at a block boundary, exactly on chunk j's start bit:
// then its start was a real boundary of the real stream, its unknown symbols are resolved from chunk j-1's last 32 KiB, and
// the member's CRC-32 is combined from the chunks' (zlib's crc32_combine).  Where the chain breaks — a false candidate, no
// candidate, a symbol buffer too small, the end of what was read — the next batch simply starts at the last boundary that
// counted.  Whatever is not the plain middle of a member is not handled here at all: in front of the final block, at a block
// that does not decode, or when a batch made no progress, the bytes so far are delivered and the one-thread reader (GzFast)
// takes the member over from that bit with the window, the CRC-32 and the length so far — so the trailer check, further
// members, trailing bytes, truncation and every message are exactly the one-thread reader's.  Regular files only.
// HULK_GZ_THREADS as for BGZF; HULK_GZ_PAR=0 switches it off; HULK_GZ_PAR_CHUNK (bytes, >= 8 KiB) for tests.
// ------------------------------------------------------------------------------------------
class GzPar : public GzStream {
 public:
    size_t chunk_bytes() const { return cfg_.gz_chunk; }
    // worth its threads and its scratch (2 T symbol buffers of ~21 chunk sizes each) from 4 chunks of compressed input on
    static bool wanted(int fd, const IngestCfg &cfg) {
        struct stat sb;
        return cfg.gz_par && cfg.gz_threads > 1 && fstat(fd, &sb) == 0 && (size_t)sb.st_size >= 4 * cfg.gz_chunk;
    }
    GzPar(int fd, const IngestCfg &cfg) : cfg_(cfg), fd_(fd), t_start_(clock_s()) {
        // no more chunks per batch than the file has: a 5 MB file does not map the scratch of 16 decoders
        struct stat sb;
        if (fstat(fd, &sb) == 0) cfg_.gz_threads = (unsigned)std::max<size_t>(2, std::min<size_t>(cfg_.gz_threads, (size_t)sb.st_size / cfg_.gz_chunk));
        th_ = std::thread([this] { produce(); t_done_ = clock_s() - t_start_; });
    }
    static double clock_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    ~GzPar() override {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        cv_.notify_all();
        const double t_close = clock_s() - t_start_;
        if (th_.joinable()) th_.join();
        if (cfg_.trace)
            fprintf(stderr, "ingest trace: parallel gzip reader timeline (s since it was opened): first batch out %.3f, last batch out %.3f, producer gone %.3f, "
                    "reader closed %.3f\n", t_first_, t_last_, t_done_, t_close);
        if (cfg_.trace)
            fprintf(stderr, "ingest trace: parallel gzip reader, %llu batches, %llu chunks counted / %llu decoded, %llu bytes of text, %llu members ended here%s; producer s: "
                    "input %.3f, decode %.3f, windows %.3f, waiting for the batch in front to become bytes %.3f\n",
                    (unsigned long long)n_batches_, (unsigned long long)n_counted_, (unsigned long long)n_decoded_, (unsigned long long)n_bytes_,
                    (unsigned long long)n_members_, tail_ ? ", then handed over to the one-thread reader" : "", t_in_, t_dec_, t_win_, t_fin_);
        if (tail_) tail_.reset();                                  // (owns and closes the descriptor from then on)
        else if (fd_ > 0) ::close(fd_);
    }
    long read(uint8_t *dst, size_t cap, std::string &msg) override {
        for (;;) {
            if (tail_) return tail_->read(dst, cap, msg);
            if (!cur_) {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [this] { return !ready_.empty(); });
                cur_ = ready_.front(); ready_.pop_front();
            }
            if (cur_->off < cur_->out_len) {
                const size_t n = std::min(cap, cur_->out_len - cur_->off);
                copy_wide(dst, cur_->out.as<uint8_t>() + cur_->off, n);
                cur_->off += n;
                return (long)n;
            }
            if (!cur_->err.empty()) { msg = cur_->err; return -1; }
            if (cur_->hand) {
                if (::lseek(fd_, cur_->hand_off, SEEK_SET) < 0) { msg = std::string("lseek: ") + strerror(errno); return -1; }
                tail_.reset(cur_->mid_member ? new GzFast(fd_, false, &cur_->resume) : new GzFast(fd_, cur_->stream_start));
                continue;
            }
            { std::lock_guard<std::mutex> g(m_); free_.push_back(cur_); }
            cv_.notify_all();
            cur_ = nullptr;
        }
    }

 private:
    IngestCfg cfg_;                                          // this run's knobs (resolve_cfg)
    static constexpr size_t W = hulk::inflate::SPEC_WINDOW;
    static constexpr int64_t PENDING = -1, NONE = -2;
    struct Batch {
        BigBuf out; size_t out_cap = 0, out_len = 0, off = 0;
        // hand-over to the one-thread reader at byte hand_off: inside a member (resume), or in front of a member's header —
        // the first of the stream (a bad header is an error) or not (it is the clean end)
        bool hand = false, mid_member = false, stream_start = false; off_t hand_off = 0; GzResume resume; std::string err;
    };
    Batch *get_free() {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [this] { return !free_.empty() || stop_; });
        if (stop_) return nullptr;
        Batch *b = free_.back(); free_.pop_back();
        b->out_len = b->off = 0; b->hand = b->mid_member = b->stream_start = false; b->err.clear();
        return b;
    }
    void publish(Batch *b) {
        t_last_ = clock_s() - t_start_; if (t_first_ < 0) t_first_ = t_last_;
        { std::lock_guard<std::mutex> g(m_); ready_.push_back(b); } cv_.notify_all();
    }
    static long pread_all(int fd, uint8_t *dst, size_t len, off_t at) {
        size_t got = 0;
        while (got < len) {
            const ssize_t m = ::pread(fd, dst + got, len - got, at + (off_t)got);
            if (m < 0) { if (errno == EINTR) continue; return -1; }
            if (m == 0) break;
            got += (size_t)m;
        }
        return (long)got;
    }
    // length of the gzip header at p (n bytes there), 0 = not all there / not one
    static size_t header_len(const uint8_t *p, size_t n) {
        if (n < 10 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8) return 0;
        const uint8_t flg = p[3];
        size_t o = 10;
        if (flg & 4) { if (o + 2 > n) return 0; o += 2 + ((size_t)p[o] | ((size_t)p[o + 1] << 8)); if (o > n) return 0; }
        if (flg & 8) { while (o < n && p[o]) o++; if (o >= n) return 0; o++; }
        if (flg & 16) { while (o < n && p[o]) o++; if (o >= n) return 0; o++; }
        if (flg & 2) { o += 2; }
        return o <= n ? o : 0;
    }

    void produce() {
        using namespace hulk::inflate;
        const unsigned T = cfg_.gz_threads;
        const unsigned HW = std::max(1u, std::thread::hardware_concurrency());
        const size_t C = chunk_bytes(), EXTRA = std::max<size_t>(C, 1u << 20), IN_LEN = (size_t)T * C + EXTRA;
        // symbols per chunk: FASTQ deflates 3-5x; a block of zlib's is <= 32 Ki symbols of <= 258 bytes.  Where a chunk does not fit
        // the chain breaks, no more — but a file that keeps breaking it (text that deflates 10x and more) is decoded T times for
        // nothing: after three batches in a row of which less than half counted, the one-thread reader gets the rest
        const size_t CAP = std::max<size_t>(10 * C, 2u << 20);
        unsigned poor = 0;
        // the gzip header
        uint64_t q;                                                // bit of the file where the next batch starts (a block boundary)
        {
            std::vector<uint8_t> h(1u << 16);
            const long m = pread_all(fd_, h.data(), h.size(), 0);
            const size_t hl = m > 0 ? header_len(h.data(), (size_t)m) : 0;
            if (hl == 0) {                                         // the one-thread reader says what is wrong with it
                Batch *b = get_free(); if (!b) return;
                b->hand = true; b->mid_member = false; b->stream_start = true; b->hand_off = 0; publish(b); return;
            }
            q = 8 * (uint64_t)hl;
        }
        BigBuf inbuf[2];
        // Two sets of symbol buffers / tables: while the chunks of batch k+1 are decoded into one, the symbols of batch k are
        // turned into bytes out of the other (all that batch k+1 needs of batch k is where it ended and its last 32 KiB,
        // which the cheap window pass delivers).  Not initialised: pages are touched as far as a chunk gets.
        struct Set { std::vector<BigBuf> sym; std::vector<SpecChunk> ch; std::vector<uint8_t> lut; };
        Set sets[2];
        try {
            for (auto &ib : inbuf) ib.reset(IN_LEN + SPEC_IN_SLACK);
            for (auto &st : sets) {
                st.sym = std::vector<BigBuf>(T); st.ch.resize(T); st.lut.resize((size_t)T * (256 + W));
                for (auto &p : st.sym) p.reset(2 * (W + CAP + SPEC_OUT_SLACK + 8));
            }
        } catch (const std::bad_alloc &) {                       // no room for the scratch (address space, not pages): one thread needs none
            Batch *b = get_free(); if (!b) return;
            b->hand = true; b->mid_member = false; b->stream_start = true; b->hand_off = 0; publish(b); return;
        }
        std::vector<std::atomic<int64_t>> start(T + 1);
        std::vector<uint8_t> win(W, 0);
        size_t have = 0; uint64_t total_ahead = 0;               // (text in front of the batch being decoded)
        uint32_t crc = 0; uint64_t total = 0;                    // of the text handed to the consumer: the finisher's
        // the next batch's input is read ahead while this one is decoded (its position is a guess: this batch's nominal end)
        int cur_in = 0;
        Team decoders(T - 1), resolvers(std::min(HW, 4 * T) - 1);   // (declared in front of the threads that use them: gone after those)
        std::thread ahead; off_t ahead_off = -1; long ahead_got = 0; int ahead_errno = 0;
        std::thread finisher;
        bool gone = false;                                        // the consumer went away while a finisher waited for a free batch
        bool at_final = false, give_up_final = false;
        struct Joiner { std::thread &a, &b; ~Joiner() { if (a.joinable()) a.join(); if (b.joinable()) b.join(); } } joiner{ahead, finisher};
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };

        for (uint64_t k = 0;; k++) {
            Set &S = sets[k & 1];
            // the first batch of a file is a quarter of the others: the parser and the GPU behind this reader start that much sooner
            const unsigned nmax = k == 0 ? std::max(2u, T / 4) : T;
            double t0 = now();
            // input: from the read-ahead when the guess was good, else read now
            if (ahead.joinable()) ahead.join();
            const off_t qb = (off_t)(q >> 3);
            off_t F; long got;
            // (good = the batch starts in the first half of the first chunk of what was read ahead)
            int read_errno = 0;
            if (ahead_off >= 0 && qb >= ahead_off && (size_t)(qb - ahead_off) < std::min(EXTRA, C) / 2) { cur_in ^= 1; F = ahead_off; got = ahead_got; read_errno = ahead_errno; }
            else { F = qb; got = pread_all(fd_, inbuf[cur_in].as<uint8_t>(), IN_LEN, F); read_errno = errno; }
            ahead_off = -1;
            uint8_t *in = inbuf[cur_in].as<uint8_t>();
            if (got >= 0) memset(in + got, 0, SPEC_IN_SLACK);
            const uint64_t in_bits = got > 0 ? 8 * (uint64_t)got : 0, bit0 = q - 8 * (uint64_t)F;
            const bool no_input = got < 0 || in_bits < bit0 + 3;
            if (!no_input && (size_t)got == IN_LEN) {
                ahead_off = F + (off_t)((size_t)nmax * C);
                uint8_t *dst = inbuf[cur_in ^ 1].as<uint8_t>();
                ahead = std::thread([this, dst, IN_LEN, ahead_off, &ahead_got, &ahead_errno] { ahead_got = pread_all(fd_, dst, IN_LEN, ahead_off); ahead_errno = errno; });
            }
            t_in_ += now() - t0; t0 = now();
            if (at_final && !no_input) {
                // The chain arrived in front of the member's final block.  One block, decoded here with the window that is known now;
                // then the trailer is checked against the combined CRC-32 and the length, and if a gzip header follows, the next
                // member is this reader's too.  Anything else about it — the block does not decode, does not end inside what was read, a
                // wrong trailer — and the one-thread reader gets the member from the bit in front of the block, as if this had not been tried.
                at_final = false;
                SpecChunk &c = S.ch[0];
                // (the zero bytes behind the input count as input for the decoder's look-ahead — a final block at the very end of the file
                // has only the 8 trailer bytes behind it —: a stream that really goes on into them fails the position test below)
                c.in = in; c.in_bits = in_bits + 8 * IN_SLACK; c.base = S.sym[0].as<uint16_t>() + W; c.cap = CAP; c.out_len = 0; c.stop = SPEC_ERROR;
                static_assert(IN_SLACK + 8 <= SPEC_IN_SLACK, "the decoder's look-ahead fits the padding behind the input");
                for (size_t i = 0; i < W; i++) c.base[(ptrdiff_t)i - (ptrdiff_t)W] = win[i];
                c.hist_have = have;
                spec_run(c, bit0, [](uint64_t) { return false; }, true);
                const uint64_t tr = (c.end_bit + 7) & ~(uint64_t)7;                 // the trailer, behind the next byte boundary
                bool ok = c.stop == SPEC_LINK && c.blocks == 1 && tr + 64 <= in_bits;
                if (finisher.joinable()) finisher.join();                            // (crc / total are final now)
                if (gone) return;
                Batch *b = nullptr;
                uint32_t crc_all = 0;
                if (ok) {
                    b = get_free();
                    if (!b) return;
                    try {
                        if (b->out_cap < c.out_len) { b->out_cap = 0; b->out.reset(c.out_len + 64); b->out_cap = c.out_len; }
                    } catch (const std::bad_alloc &) {
                        b->out_len = 0; b->err = "gzip: out of memory for " + std::to_string(c.out_len) + " bytes of inflated text";
                        publish(b); return;
                    }
                    uint8_t *l = S.lut.data();
                    for (int i = 0; i < 256; i++) l[i] = (uint8_t)i;
                    memcpy(l + 256, win.data(), W);
                    spec_resolve(c.base, c.out_len, l, b->out.as<uint8_t>());
                    crc_all = (uint32_t)crc32_combine(crc, hulk::crc32_fast(0, b->out.as<uint8_t>(), c.out_len), (z_off_t)c.out_len);
                    const uint8_t *t = in + (tr >> 3);
                    const uint32_t want_crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
                    const uint32_t want_size = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
                    ok = crc_all == want_crc && (uint32_t)(total + c.out_len) == want_size;
                    if (!ok) { std::lock_guard<std::mutex> g(m_); free_.push_back(b); b = nullptr; }
                }
                if (ok) {
                    b->out_len = c.out_len; n_bytes_ += c.out_len; n_members_++;
                    const size_t after = (size_t)(tr >> 3) + 8;                      // first byte behind the trailer, in the buffer
                    const size_t hl = header_len(in + after, (size_t)got - after);
                    // a new member: no window, no checksum, no length
                    crc = 0; total = 0; total_ahead = 0; have = 0;
                    if (hl == 0) {                                                    // no header, or not all of it here: the one-thread reader's
                        b->hand = true; b->mid_member = false; b->stream_start = false; b->hand_off = F + (off_t)after;
                        publish(b);
                        return;
                    }
                    publish(b);
                    q = 8 * ((uint64_t)F + after + hl);
                    continue;
                }
                // (falls through: the ordinary path finds SPEC_FINAL at once, counts nothing, and hands the member over at q)
                give_up_final = true;
            }
            unsigned n = 0, acc = 0;
            std::vector<size_t> off(1, 0);
            uint64_t q_new = q;
            SpecStop last_stop = SPEC_INPUT;
            if (!no_input) {
                n = (unsigned)std::min<size_t>(nmax, ((size_t)got + C - 1) / C);
                for (unsigned j = 0; j <= n; j++) start[j].store(j == 0 ? (int64_t)bit0 : PENDING, std::memory_order_relaxed);
                auto decode = [&](unsigned j) {
                    SpecChunk &c = S.ch[j];
                    c.in = in; c.in_bits = in_bits; c.base = S.sym[j].as<uint16_t>() + W; c.cap = CAP; c.out_len = 0; c.stop = SPEC_ERROR;
                    uint64_t s = bit0;
                    if (j > 0) {
                        const uint64_t from = std::max<uint64_t>(8 * (uint64_t)j * C, bit0 + 1);
                        s = find_block_start(in, in_bits, from, 8 * (uint64_t)j * C + 4 * (uint64_t)C);
                        start[j].store(s == ~0ull ? NONE : (int64_t)s, std::memory_order_release);
                        if (s == ~0ull) return;
                        for (size_t i = 0; i < W; i++) c.base[(ptrdiff_t)i - (ptrdiff_t)W] = (uint16_t)(256 + i);
                        c.hist_have = W;
                    } else {
                        for (size_t i = 0; i < W; i++) c.base[(ptrdiff_t)i - (ptrdiff_t)W] = win[i];
                        c.hist_have = have;
                    }
                    const uint64_t nominal_end = 8 * (uint64_t)(j + 1) * C;
                    spec_run(c, s, [&](uint64_t pos) {
                        if (pos < nominal_end) return false;
                        if (j + 1 >= n) return true;
                        int64_t nx;
                        while ((nx = start[j + 1].load(std::memory_order_acquire)) == PENDING) std::this_thread::yield();
                        return nx == NONE || pos >= (uint64_t)nx;
                    });
                };
                decoders.run(n, decode);
                t_dec_ += now() - t0; t0 = now();
                // the chain: which chunks count
                uint64_t cum = total_ahead;
                for (unsigned j = 0; j < n; j++) {
                    if (j > 0) {
                        const int64_t sj = start[j].load(std::memory_order_relaxed);
                        if (sj < 0 || S.ch[j - 1].stop != SPEC_LINK || S.ch[j - 1].end_bit != (uint64_t)sj || cum < W) break;
                    }
                    acc++; cum += S.ch[j].out_len;
                }
                n_batches_++; n_counted_ += acc; n_decoded_ += n;
                q_new = 8 * (uint64_t)F + S.ch[acc - 1].end_bit;
                last_stop = S.ch[acc - 1].stop;
                // the windows, in order (cheap): table j = identity + the 32 KiB in front of chunk j
                off.assign(acc + 1, 0);
                for (unsigned j = 0; j < acc; j++) {
                    uint8_t *l = S.lut.data() + (size_t)j * (256 + W);
                    for (int i = 0; i < 256; i++) l[i] = (uint8_t)i;
                    memcpy(l + 256, win.data(), W);
                    const uint16_t *e = S.ch[j].base + S.ch[j].out_len;  // (reaches into the window in front of the symbols when the chunk is short)
                    for (size_t i = 0; i < W; i++) win[i] = l[e[(ptrdiff_t)i - (ptrdiff_t)W]];
                    have = std::min(W, have + S.ch[j].out_len);
                    off[j + 1] = off[j] + S.ch[j].out_len;
                }
                total_ahead += off[acc];
                t_win_ += now() - t0; t0 = now();
            }
            const bool stuck = q_new == q;
            q = q_new;
            poor = 2 * acc < n ? poor + 1 : 0;
            // in front of the final block with everything else in order: the next round of this loop tries the member's end
            if (!no_input && last_stop == SPEC_FINAL && !give_up_final && !(poor >= 3)) at_final = true;
            const bool hand = no_input || (last_stop == SPEC_FINAL && !at_final) || last_stop == SPEC_ERROR || (stuck && !at_final) || poor >= 3;
            give_up_final = false;
            // the batch in front has to be out of its symbol buffers (the next decode writes them) and its checksum final
            if (finisher.joinable()) finisher.join();
            t_fin_ += now() - t0;
            if (gone) return;
            GzResume res;
            if (hand) { res.bit = (int)(q & 7); res.hist.assign(win.end() - (ptrdiff_t)have, win.end()); }
            const std::string io_err = got < 0 ? std::string("read: ") + strerror(read_errno) : std::string();
            // bytes and checksums, side by side in pieces of >= 256 KiB, while the next batch is decoded
            finisher = std::thread([this, &S, &crc, &total, &gone, &resolvers, off = std::move(off), acc, hand, res = std::move(res), io_err, q, HW, T]() mutable {
                Batch *b = get_free();
                if (!b) { gone = true; return; }
                const size_t out_total = off[acc];
                struct Piece { unsigned j; size_t at, len; uint32_t crc; };
                std::vector<Piece> pieces;
                // (this thread has no caller to unwind to: running out of memory here must end the run with a message, not the
                //  process with std::terminate — ADVICE r3)
                try {
                    if (b->out_cap < out_total) { b->out_cap = 0; b->out.reset(out_total + out_total / 16 + 64); b->out_cap = out_total + out_total / 16; }
                    pieces.reserve(acc * 8 + 64);
                } catch (const std::bad_alloc &) {
                    b->out_len = 0; b->err = "gzip: out of memory for " + std::to_string(out_total) + " bytes of inflated text";
                    publish(b); gone = true; return;
                }
                const size_t target = std::max<size_t>(256u << 10, out_total / std::max(1u, std::min(HW, 4 * T)) + 1);
                for (unsigned j = 0; j < acc; j++) {
                    const size_t len = S.ch[j].out_len, parts = std::max<size_t>(1, len / target), step = ((len + parts - 1) / parts + 63) & ~(size_t)63;
                    for (size_t at = 0; at < len; at += step) pieces.push_back({j, at, std::min(step, len - at), 0});
                }
                std::atomic<size_t> next{0};
                auto work = [&] {
                    for (size_t i; (i = next.fetch_add(1)) < pieces.size();) {
                        Piece &pc = pieces[i];
                        uint8_t *dst = b->out.as<uint8_t>() + off[pc.j] + pc.at;
                        hulk::inflate::spec_resolve(S.ch[pc.j].base + pc.at, pc.len, S.lut.data() + (size_t)pc.j * (256 + W), dst);
                        pc.crc = hulk::crc32_fast(0, dst, pc.len);
                    }
                };
                resolvers.run((unsigned)std::min<size_t>(pieces.size(), resolvers.size()), [&](unsigned) { work(); });
                for (const Piece &pc : pieces) crc = (uint32_t)crc32_combine(crc, pc.crc, (z_off_t)pc.len);
                total += out_total; n_bytes_ += out_total;
                b->out_len = out_total;
                if (!io_err.empty()) b->err = io_err;
                else if (hand) {
                    b->hand = true; b->mid_member = true; b->hand_off = (off_t)(q >> 3);
                    b->resume = std::move(res); b->resume.crc = crc; b->resume.size = (uint32_t)total;
                }
                publish(b);
            });
            if (hand || !io_err.empty()) return;                   // (the Joiner waits for the finisher)
        }
    }

    int fd_;
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    Batch batches_[3];
    std::deque<Batch *> free_{&batches_[0], &batches_[1], &batches_[2]}, ready_;
    bool stop_ = false;
    Batch *cur_ = nullptr;
    std::unique_ptr<GzFast> tail_;
    uint64_t n_batches_ = 0, n_counted_ = 0, n_decoded_ = 0, n_bytes_ = 0, n_members_ = 0;
    double t_in_ = 0, t_dec_ = 0, t_win_ = 0, t_fin_ = 0;
    double t_start_ = 0, t_first_ = -1, t_last_ = 0, t_done_ = 0;
};

}  // namespace

std::unique_ptr<GzStream> gz_open(int fd, bool regular, const IngestCfg &cfg) {
    if (cfg.zlib) {
        gzFile gz = gzdopen(fd, "rb");
        return std::unique_ptr<GzStream>(gz ? new GzZlib(gz) : nullptr);
    }
    if (regular && cfg.gz_threads > 1 && GzBgzf::looks_like(fd)) return std::unique_ptr<GzStream>(new GzBgzf(fd, cfg));
    if (regular && GzPar::wanted(fd, cfg)) return std::unique_ptr<GzStream>(new GzPar(fd, cfg));
    return std::unique_ptr<GzStream>(new GzFast(fd));
}
std::unique_ptr<GzStream> gz_open_sequential(int fd, bool first) { return std::unique_ptr<GzStream>(new GzFast(fd, first)); }

}  // namespace ingest
}  // namespace hulk
