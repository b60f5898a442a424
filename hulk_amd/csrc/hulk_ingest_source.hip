// Where the bytes of a run come from (hulk_ingest.h): the process's pool of large host regions, the sequential byte source over
// the inputs (files, gzip, STDIN) and the block reader of the host parser.  The context is not used here; of the HIP runtime only
// what hulk::bgzf::DevReader does behind its interface.
#include <errno.h>
#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

#include "hulk_ingest.h"
#include "hulk_internal.h"
#include "hulk_bgzf.h"

namespace hulk {
namespace ingest {

// ---- RegionPool / BigBuf (hulk_ingest.h has the why) ----
void *RegionPool::take(size_t n) {
    std::lock_guard<std::mutex> g(mu);
    for (size_t i = v.size(); i-- > 0;)
        if (v[i].n == n) { void *p = v[i].p; bytes -= n; v.erase(v.begin() + i); return p; }
    return nullptr;
}
bool RegionPool::give(void *p, size_t n) {
    static const bool off = HULK_EXP_ENV("HULK_NO_REGION_POOL") != nullptr;
    if (off || n > ONE_MAX) return false;
    std::lock_guard<std::mutex> g(mu);
    if (bytes + n > POOL_BYTES) return false;
    v.push_back({p, n, now()}); bytes += n;
    return true;
}
void RegionPool::sweep(double older_than) {
    std::vector<Ent> drop;
    {
        std::lock_guard<std::mutex> g(mu);
        const double t = now();
        for (size_t i = 0; i < v.size();)
            if (t - v[i].t >= older_than) { drop.push_back(v[i]); bytes -= v[i].n; v.erase(v.begin() + i); } else i++;
    }
    for (auto &e : drop) ::munmap(e.p, e.n);
}
void BigBuf::release() { if (p && !RegionPool::get().give(p, n)) ::munmap(p, n); p = nullptr; n = 0; }
void BigBuf::reset(size_t bytes) {
    release();
    n = (bytes + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
    if ((p = RegionPool::get().take(n))) return;
    void *m = ::mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) { p = nullptr; n = 0; throw std::bad_alloc(); }
    p = m;
    static const bool thp = HULK_EXP_ENV("HULK_GZ_NO_THP") == nullptr;
    if (thp) ::madvise(p, n, MADV_HUGEPAGE);
}

// ---- ByteSource ----
ByteSource::ByteSource(const char *const *paths, uint32_t n, const IngestCfg &cfg) : cfg_(cfg) {
    for (uint32_t i = 0; i < n; i++) paths_.push_back(paths[i] ? paths[i] : "");
    stdin_mode_ = paths_.empty();
}
ByteSource::~ByteSource() { close_current(); }

long ByteSource::read(uint8_t *dst, size_t cap, IngestError &err, uint8_t *ddst, bool *on_dev) {
    if (on_dev) *on_dev = false;
    for (;;) {
        if (!open_) {
            if (stdin_mode_) { if (stdin_done_) return 0; fd_ = 0; open_ = true; }
            else {
                if (idx_ >= paths_.size()) return 0;
                if (!open_path(paths_[idx_], err)) return -1;
            }
            last_ = '\n'; got_any_ = false;
        }
        long n;
        if (gzf_) {
            std::string msg;
            n = gzf_->read(dst, cap, msg);
            if (n < 0) { err.set(HULK_ERR_IO, msg); return -1; }
        } else if (dgz_) {
            std::string msg;
            uint8_t last = last_;
            n = dgz_->read(ddst, cap, &last, msg);
            if (n < 0) { err.set(HULK_ERR_HIP, msg); return -1; }
            if (n > 0) { last_ = last; got_any_ = true; *on_dev = true; return n; }
            if (dgz_->hand_over() >= 0) {                  // the rest of the file is the sequential reader's (GzBgzf's rule)
                if (::lseek(fd_, dgz_->hand_over(), SEEK_SET) < 0) { err.set(HULK_ERR_IO, std::string("lseek: ") + strerror(errno)); return -1; }
                gzf_ = gz_open_sequential(fd_, !dgz_->any_member());
                continue;
            }
        } else if (regular_ && cap >= PAR_READ_MIN && readers() > 1) {
            n = read_pieces(dst, cap);
            if (n < 0) { err.set(HULK_ERR_IO, std::string("read ") + current_name() + ": " + strerror(errno)); return -1; }
        } else {
            do { n = regular_ ? ::pread(fd_, dst, cap, pos_) : ::read(fd_, dst, cap); } while (n < 0 && errno == EINTR);
            if (n < 0) { err.set(HULK_ERR_IO, std::string("read ") + current_name() + ": " + strerror(errno)); return -1; }
            pos_ += (off_t)n;
        }
        if (n > 0) { last_ = dst[n - 1]; got_any_ = true; return n; }
        // end of this input
        const bool need_nl = got_any_ && last_ != '\n';
        close_current();
        if (stdin_mode_) stdin_done_ = true; else idx_++;
        if (need_nl) { dst[0] = '\n'; return 1; }
    }
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
long ByteSource::read_pieces(uint8_t *dst, size_t cap) {
    const unsigned R = readers();
    const size_t piece = (cap / R + 4095) & ~(size_t)4095;
    std::vector<long> got(R, 0);
    std::vector<int> errs(R, 0);
    if (!team_) team_.reset(new Team(R - 1));
    team_->run(R, [&](unsigned i) {
        const size_t at = (size_t)i * piece;
        if (at >= cap) return;
        got[i] = pread_all(fd_, dst + at, std::min(piece, cap - at), pos_ + (off_t)at);
        if (got[i] < 0) errs[i] = errno;
    });
    size_t total = 0;
    for (unsigned i = 0; i < R; i++) {
        if (got[i] < 0) { errno = errs[i]; return -1; }
        total += (size_t)got[i];
        const size_t at = (size_t)i * piece;
        if (at >= cap || (size_t)got[i] < std::min(piece, cap - at)) break;      // end of file inside this piece
    }
    pos_ += (off_t)total;
    return (long)total;
}
bool ByteSource::open_path(const std::string &p, IngestError &err) {
    fd_ = ::open(p.c_str(), O_RDONLY);
    if (fd_ < 0) return err.set(HULK_ERR_IO, "open " + p + ": " + strerror(errno));   // os.Open's *PathError text
    open_ = true; pos_ = 0;
    struct stat sb;
    regular_ = fstat(fd_, &sb) == 0 && S_ISREG(sb.st_mode);
    // sketch.go:64-65: strings.Split(name, ".") last element == "gz"
    const size_t dot = p.rfind('.');
    if (dot != std::string::npos && p.compare(dot + 1, std::string::npos, "gz") == 0) {
        uint8_t magic[2] = {0, 0};
        const ssize_t m = ::pread(fd_, magic, 2, 0);
        if (m == 0) { close_current(); return err.set(HULK_ERR_IO, "EOF"); }                    // gzip.NewReader on an empty file
        if (m < 2 || magic[0] != 0x1f || magic[1] != 0x8b) { close_current(); return err.set(HULK_ERR_IO, "gzip: invalid header"); }
        if (!cfg_.zlib && regular_ && dev_bufs_ && hulk::bgzf::DevReader::looks_like(fd_)) { dgz_.reset(new hulk::bgzf::DevReader(fd_, dev_bufs_, cfg_.trace)); return true; }
        gzf_ = gz_open(fd_, regular_, cfg_);
        if (!gzf_) { close_current(); return err.set(HULK_ERR_IO, "gzip: cannot open stream"); }
    }
    return true;
}
void ByteSource::close_current() {
    dgz_.reset();                                             // (the device reader does not own the descriptor)
    if (gzf_) { gzf_.reset(); fd_ = -1; }                     // (the gzip readers close the descriptor)
    else if (fd_ > 0) ::close(fd_);
    fd_ = -1; open_ = false;
}

// ---- BlockReader ----
BlockReader::BlockReader(const char *const *paths, uint32_t n, const IngestCfg &cfg) : block_(cfg.block), src_(paths, n, cfg) { th_ = std::thread([this] { run(); }); }
BlockReader::~BlockReader() {
    { std::lock_guard<std::mutex> g(m_); stop_ = true; }
    cv_.notify_all();
    if (th_.joinable()) th_.join();
}
std::unique_ptr<Block> BlockReader::next(IngestError &err) {
    std::unique_lock<std::mutex> g(m_);
    cv_.wait(g, [this] { return !q_.empty() || done_; });
    if (!q_.empty()) { auto b = std::move(q_.front()); q_.pop_front(); cv_.notify_all(); return b; }
    if (err_.code != HULK_OK) err = err_;
    return nullptr;
}
void BlockReader::recycle(std::unique_ptr<Block> b) { std::lock_guard<std::mutex> g(m_); if (pool_.size() < 3) pool_.push_back(std::move(b)); }
void BlockReader::run() {
    std::vector<uint8_t> carry;
    bool eof = false;
    while (!eof) {
        std::unique_ptr<Block> b;
        {
            std::unique_lock<std::mutex> g(m_);
            cv_.wait(g, [this] { return q_.size() < 2 || stop_; });
            if (stop_) break;
            if (!pool_.empty()) { b = std::move(pool_.back()); pool_.pop_back(); }
        }
        if (!b) b.reset(new Block);
        if (b->buf.size() < block_ + MAX_TOKEN + 16) b->buf.resize(block_ + MAX_TOKEN + 16);
        size_t have = carry.size();
        if (have > b->buf.size() - block_) b->buf.resize(have + block_ + 16);
        if (have) memcpy(b->buf.data(), carry.data(), have);
        carry.clear();
        IngestError e;
        while (have < block_) {
            const long n = src_.read(b->buf.data() + have, block_ - have, e);
            if (n < 0) { finish(e); return; }
            if (n == 0) { eof = true; break; }
            have += (size_t)n; bytes_in_ += (uint64_t)n;
        }
        // cut at the last '\n'
        size_t cut = have;
        while (cut > 0 && b->buf[cut - 1] != '\n') cut--;
        b->tail_too_long = false;
        if (!eof) {
            carry.assign(b->buf.begin() + cut, b->buf.begin() + have);
            if (carry.size() >= MAX_TOKEN) b->tail_too_long = true;
        }   // at EOF every input ended in '\n' (ByteSource), so cut == have
        b->len = eof ? have : cut;
        const bool fatal_tail = b->tail_too_long;
        {
            std::lock_guard<std::mutex> g(m_);
            q_.push_back(std::move(b));
        }
        cv_.notify_all();
        if (fatal_tail) break;       // the parser reports "token too long" after this block
    }
    IngestError none;
    finish(none);
}
void BlockReader::finish(const IngestError &e) {
    { std::lock_guard<std::mutex> g(m_); err_ = e; done_ = true; }
    cv_.notify_all();
}

}  // namespace ingest
}  // namespace hulk
