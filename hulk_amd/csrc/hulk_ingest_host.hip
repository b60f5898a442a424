// Host ingest of libhulkhip: files / STDIN -> lines -> sequences -> pinned staging -> HBM.
//
// Replaces, with the same observable semantics, the reference's
//   DataStreamer.Run   src/pipeline/sketch.go:40-79   (bufio.Scanner lines; gzip when the name ends
//                                                       in ".gz"; STDIN when no file is given)
//   FastqHandler.Run   src/pipeline/sketch.go:99-161  (four nil-tested line slots; FASTA branch)
//   seqio.NewFASTQread src/seqio/seqio.go:38-40       ('@' check when the 4th line arrives)
// and the AddSeq loop of SeqMinimizer.Run (sketch.go:196-217) when a context is attached.
//
// Shape: a reader thread turns the inputs into 32 MB blocks that end on a line boundary (gzip
// inflation runs there, ahead of the parser); a block is parsed by P threads in two passes — pass 1
// runs the 4-state line machine for all four possible start states of every piece (state,
// sequences, bytes), a serial prefix fixes each piece's real start state and its output offsets,
// pass 2 copies the sequence lines straight into pinned staging — and is handed to the GPU with
// asynchronous copies on the context's stream while the next block is read and parsed.
//
// This unit is the host parsers and hulk_parse_files: it uses neither a context nor the HIP runtime.  The readers in front of it are
// hulk_ingest_gzip.hip and hulk_ingest_source.hip; the way into a context and the device parsers are hulk_ingest_device.hip.
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <algorithm>

#include "hulk_ingest.h"

namespace hulk {
namespace ingest {

IngestCfg resolve_cfg(const hulk_ingest_opts *o, uint32_t threads) {
    IngestCfg c;
    c.parser_threads = threads;
    if (o) {
        if (o->parser_threads) c.parser_threads = o->parser_threads;
        if (o->gz_threads) c.gz_threads = o->gz_threads;
        if (o->block_bytes) { c.block = (size_t)o->block_bytes; c.block_set = true; }
        if (o->gz_chunk_bytes) c.gz_chunk = (size_t)o->gz_chunk_bytes;
        if (o->file_readers) { c.readers = o->file_readers; c.readers_set = true; }
        if (o->flags & HULK_INGEST_GZ_ONE_THREAD) c.gz_par = false;
        if (o->flags & HULK_INGEST_GZ_ZLIB) c.zlib = true;
        if (o->flags & HULK_INGEST_TRACE) c.trace = true;
        if (o->flags & HULK_INGEST_HOST_PARSER) c.host_parser = true;
        if (o->flags & HULK_INGEST_DEVICE_INFLATE) c.dev_inflate = true;
    }
    if (!o || !o->gz_threads) {                   // the default of 16 inflate threads is for hosts that have them
        const long hw = (long)std::thread::hardware_concurrency();
        if (hw > 0 && (long)c.gz_threads > hw) c.gz_threads = (unsigned)hw;
    }
    if (const char *e = getenv("HULK_INGEST_BLOCK")) { c.block = (size_t)strtoull(e, nullptr, 10); c.block_set = true; }
    if (const char *e = getenv("HULK_GZ_THREADS")) c.gz_threads = (unsigned)std::max(1L, strtol(e, nullptr, 10));
    if (const char *e = getenv("HULK_GZ_PAR")) c.gz_par = !(e[0] == '0');
    if (const char *e = getenv("HULK_GZ_PAR_CHUNK")) c.gz_chunk = (size_t)strtoull(e, nullptr, 10);
    if (const char *e = getenv("HULK_GZ_DEVICE")) c.dev_inflate = !(e[0] == '0');
    if (const char *e = getenv("HULK_INGEST_READERS")) { c.readers = (unsigned)std::max(1L, strtol(e, nullptr, 10)); c.readers_set = true; }
    if (getenv("HULK_GZ_ZLIB")) c.zlib = true;
    if (getenv("HULK_INGEST_TRACE")) c.trace = true;
    if (c.block < 2 * MAX_TOKEN) c.block = 2 * MAX_TOKEN;
    if (c.gz_threads < 1) c.gz_threads = 1;
    if (c.gz_threads > 64) c.gz_threads = 64;
    if (c.gz_chunk < (8u << 10)) c.gz_chunk = 8u << 10;
    if (c.readers < 1) c.readers = 1;
    if (c.readers > 16) c.readers = 16;
    return c;
}
// hulk_ingest_opts as hulk_create checks hulk_params: unknown flags, non-zero reserved fields and values outside the ranges
// the header states are refused, not clamped (an empty string: the options are fine)
std::string check_opts(const hulk_ingest_opts *o) {
    if (!o) return std::string();
    if (o->flags & ~(HULK_INGEST_GZ_ONE_THREAD | HULK_INGEST_GZ_ZLIB | HULK_INGEST_TRACE | HULK_INGEST_HOST_PARSER | HULK_INGEST_DEVICE_INFLATE)) return "hulk_ingest_opts: unknown flags";
    if (o->reserved[0] || o->reserved[1]) return "hulk_ingest_opts: reserved must be 0";
    if (o->parser_threads > 256) return "hulk_ingest_opts: parser_threads must be 0 (default) or 1..256";
    if (o->gz_threads > 64) return "hulk_ingest_opts: gz_threads must be 0 (default) or 1..64";
    if (o->file_readers > 16) return "hulk_ingest_opts: file_readers must be 0 (default) or 1..16";
    if (o->block_bytes && o->block_bytes < 2 * MAX_TOKEN) return "hulk_ingest_opts: block_bytes must be 0 (default) or >= 128 KiB";
    if (o->block_bytes > (1ull << 31)) return "hulk_ingest_opts: block_bytes must be <= 2 GiB";
    if (o->gz_chunk_bytes && o->gz_chunk_bytes < (8u << 10)) return "hulk_ingest_opts: gz_chunk_bytes must be 0 (default) or >= 8 KiB";
    return std::string();
}
namespace {
struct CallbackSink : Sink {
    hulk_batch_fn fn; void *user;
    std::vector<uint8_t> bases; std::vector<uint64_t> lens;
    CallbackSink(hulk_batch_fn f, void *u) : fn(f), user(u) {}
    bool prepare(uint64_t n, uint64_t nbytes, uint8_t **b, uint64_t **l, IngestError &) override {
        if (bases.size() < nbytes + 16) bases.resize(nbytes + 16);
        if (lens.size() < n + 2) lens.resize(n + 2);
        *b = bases.data(); *l = lens.data();
        return true;
    }
    bool commit(uint64_t n, IngestError &err) override {
        if (n == 0) return true;
        uint64_t mn, mx;
        const uint64_t tot = lens_to_offsets(lens.data(), n, mn, mx);
        n_seqs += n; total_len += tot;
        if (fn) { const int rc = fn(user, bases.data(), lens.data(), n); if (rc != 0) return err.set(rc < 0 ? rc : HULK_ERR_ARG, "batch callback failed"); }
        return true;
    }
};

// ------------------------------------------------------------------------------------------
// FASTQ: the line machine of FastqHandler.Run.  state = number of filled slots (0..3).
//   state 0..2: an EMPTY line leaves the slot nil (skipped); a non-empty line fills it
//   state 3   : ANY line (empty too) is l4 and completes the record
// ------------------------------------------------------------------------------------------
static inline size_t line_len(const uint8_t *p, const uint8_t *nl) {     // ScanLines' dropCR
    size_t L = (size_t)(nl - p);
    if (L && p[L - 1] == '\r') L--;
    return L;
}

struct Scan1 {
    uint8_t end_state[4]; uint64_t nseq[4], nbytes[4]; uint64_t n_lines = 0; bool too_long = false;
};

static void fastq_pass1(const uint8_t *a, const uint8_t *b, Scan1 &r) {
    uint8_t st[4] = {0, 1, 2, 3};
    uint64_t ns[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0};
    const uint8_t *p = a;
    while (p < b) {
        const uint8_t *nl = (const uint8_t *)memchr(p, '\n', (size_t)(b - p));
        if (!nl) nl = b;                                   // cannot happen: pieces end in '\n'
        if ((size_t)(nl - p) >= MAX_TOKEN) { r.too_long = true; break; }
        const size_t L = line_len(p, nl);
        r.n_lines++;
        for (int h = 0; h < 4; h++) {
            const uint8_t s = st[h];
            if (s == 3) st[h] = 0;
            else if (L) { if (s == 1) { ns[h]++; nb[h] += L; } st[h] = (uint8_t)(s + 1); }
        }
        p = nl + 1;
    }
    for (int h = 0; h < 4; h++) { r.end_state[h] = st[h]; r.nseq[h] = ns[h]; r.nbytes[h] = nb[h]; }
}

struct Scan2 {
    uint64_t completed = 0;          // records completed in this piece
    bool bad_done = false;           // a record that STARTED here with a bad header completed here
    std::string bad_done_hdr;
    bool bad_pending = false;        // the record in progress at the end started here with a bad header
    std::string bad_pending_hdr;
    bool started = false;            // a header line was seen in this piece
};

static void fastq_pass2(const uint8_t *a, const uint8_t *b, uint8_t state, uint8_t *out, uint64_t *lens, Scan2 &r) {
    const uint8_t *p = a;
    bool cur_bad = false; std::string cur_hdr;
    while (p < b) {
        const uint8_t *nl = (const uint8_t *)memchr(p, '\n', (size_t)(b - p));
        if (!nl) nl = b;
        if ((size_t)(nl - p) >= MAX_TOKEN) break;          // reported from pass 1
        const size_t L = line_len(p, nl);
        if (state == 3) {
            r.completed++;
            if (cur_bad && !r.bad_done) { r.bad_done = true; r.bad_done_hdr = cur_hdr; }
            cur_bad = false; state = 0;
        } else if (L) {
            if (state == 0) {
                r.started = true;
                cur_bad = p[0] != '@';
                if (cur_bad) cur_hdr.assign((const char *)p, std::min<size_t>(L, 512));
            } else if (state == 1) {
                memcpy(out, p, L); out += L; *lens++ = (uint64_t)L;
            }
            state++;
        }
        p = nl + 1;
    }
    if (cur_bad && state != 0) { r.bad_pending = true; r.bad_pending_hdr = cur_hdr; }
}
}  // namespace

template <class F> void Parser::run_parallel(uint32_t P, F f) {
    if (P == 1) { f(0); return; }
    if (!team_ || team_->size() < P) team_.reset(new Team(P - 1));
    team_->run(P, [&](unsigned i) { f((uint32_t)i); });
}

// ---- FASTQ ----
bool Parser::fastq_bytes(const uint8_t *base, size_t blen, bool tail_too_long) {
    const uint8_t *end = base + blen;
    uint32_t P = (uint32_t)std::min<size_t>(threads, std::max<size_t>(1, blen / 16384));
    std::vector<const uint8_t *> cutp(P + 1);
    cutp[0] = base; cutp[P] = end;
    for (uint32_t i = 1; i < P; i++) {
        const uint8_t *q = base + blen * i / P;
        if (q < cutp[i - 1]) q = cutp[i - 1];
        const uint8_t *nl = q < end ? (const uint8_t *)memchr(q, '\n', (size_t)(end - q)) : nullptr;
        cutp[i] = nl ? nl + 1 : end;
    }
    std::vector<Scan1> s1(P);
    run_parallel(P, [&](uint32_t i) { fastq_pass1(cutp[i], cutp[i + 1], s1[i]); });
    // serial prefix: real start state and output offsets of every piece
    std::vector<uint8_t> st(P + 1);
    std::vector<uint64_t> seq0(P + 1), byte0(P + 1);
    st[0] = fq_state; seq0[0] = have_pending ? 1 : 0; byte0[0] = have_pending ? pending.size() : 0;
    for (uint32_t i = 0; i < P; i++) {
        st[i + 1] = s1[i].end_state[st[i]];
        seq0[i + 1] = seq0[i] + s1[i].nseq[st[i]];
        byte0[i + 1] = byte0[i] + s1[i].nbytes[st[i]];
        n_lines += s1[i].n_lines;
    }
    uint8_t *ob = nullptr; uint64_t *ol = nullptr;
    if (!sink.prepare(seq0[P], byte0[P], &ob, &ol, err)) return false;
    if (have_pending) { memcpy(ob, pending.data(), pending.size()); ol[0] = pending.size(); }
    std::vector<Scan2> s2(P);
    run_parallel(P, [&](uint32_t i) { fastq_pass2(cutp[i], cutp[i + 1], st[i], ob + byte0[i], ol + seq0[i], s2[i]); });
    // errors in stream order (seqio.go:38-40 fires when the record's 4th line arrives)
    for (uint32_t i = 0; i < P; i++) {
        if (carry_bad && s2[i].completed) return bad_id(carry_hdr);
        if (s2[i].bad_done) return bad_id(s2[i].bad_done_hdr);
        if (s2[i].started || s2[i].completed) { carry_bad = s2[i].bad_pending; carry_hdr = s2[i].bad_pending_hdr; }
        if (s1[i].too_long) return err.set(HULK_ERR_LINE_TOO_LONG, hulk_strerror(HULK_ERR_LINE_TOO_LONG));
    }
    if (tail_too_long) return err.set(HULK_ERR_LINE_TOO_LONG, hulk_strerror(HULK_ERR_LINE_TOO_LONG));
    fq_state = st[P];
    // a record whose sequence line has been seen but not its 4th line is not a read yet
    uint64_t n = seq0[P];
    if (fq_state >= 2 && n > 0) {
        const uint64_t L = ol[n - 1];
        uint64_t off = byte0[P] - L;
        pending.assign(ob + off, ob + off + L);
        have_pending = true; n--;
    } else if (fq_state < 2) {
        have_pending = false;
    }
    return sink.commit(n, err);
}
bool Parser::bad_id(const std::string &hdr) {
    return err.set(HULK_ERR_FASTQ_ID, std::string("read ID in fastq file does not begin with @: ") + hdr);
}

// ---- FASTA (sketch.go:102-135: the sequence lines of a '>' record concatenated; an EMPTY line ends the parsing) ----
// Records are unbounded, lines are not.  A block is cut into pieces at line ends; the pieces are parsed side by side — every
// piece compacts its sequence lines into a buffer of its own and notes where header lines fell — and copied side by side to
// the end of `fa_bases`; what is left to do in stream order is a walk over the (few) headers.  (Until round 6: one thread,
// one std::vector::insert per 60-byte line — 1.6 GB/s of file, 20x below what the long-sequence kernels take.)
Parser::RawBuf::~RawBuf() { if (p && !(cap == FIRST && RegionPool::get().give(p, cap))) ::munmap(p, cap); }
uint8_t *Parser::RawBuf::grow(size_t add) {
    if (n + add > cap) {
        const size_t nc = (std::max(std::max(cap * 2, FIRST), n + add + 4096) + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
        void *q = p ? ::mremap(p, cap, nc, MREMAP_MAYMOVE) : (nc == FIRST ? RegionPool::get().take(nc) : nullptr);
        if (!q) {
            q = ::mmap(nullptr, nc, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
            if (q != MAP_FAILED) ::madvise(q, nc, MADV_HUGEPAGE);
        } else if (p && q != MAP_FAILED) ::madvise(q, nc, MADV_HUGEPAGE);
        if (q == MAP_FAILED) throw std::bad_alloc();
        p = (uint8_t *)q; cap = nc;
    }
    uint8_t *r = p + n; n += add; return r;
}

bool Parser::fasta_flush_batch(bool final_record) {
    // everything but the record still being accumulated
    uint64_t n = fa_lens.size(), nbytes = fa_bases.size() - (final_record ? 0 : fa_cur);
    if (n == 0) return true;
    uint8_t *ob; uint64_t *ol;
    if (!sink.prepare(n, nbytes, &ob, &ol, err)) return false;
    if (nbytes >= (8u << 20) && threads > 1) {                      // (one core copies ~10 GB/s)
        const uint32_t T = std::min<uint32_t>(threads, 8);
        const size_t piece = ((nbytes + T - 1) / T + 63) & ~(size_t)63;
        run_parallel(T, [&](uint32_t t) { const size_t at = (size_t)t * piece; if (at < nbytes) memcpy(ob + at, fa_bases.p + at, std::min(piece, (size_t)nbytes - at)); });
    } else if (nbytes) memcpy(ob, fa_bases.p, nbytes);
    memcpy(ol, fa_lens.data(), n * 8);
    if (!sink.commit(n, err)) return false;
    fa_bases.erase_front(nbytes);
    fa_lens.clear();
    return true;
}
static void fasta_piece(const uint8_t *p, const uint8_t *end, Parser::FaPiece &r) {
    if ((size_t)(end - p) + 1 > r.cap) { r.cap = (size_t)(end - p) + 1 + ((size_t)(end - p) >> 3); r.buf.reset(new BigBuf(r.cap)); }
    r.hdr_at.clear(); r.n_lines = 0; r.stopped = r.too_long = false;
    uint8_t *out = r.buf->as<uint8_t>();
    while (p < end) {
        const uint8_t *nl = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
        if (!nl) nl = end;
        if ((size_t)(nl - p) >= MAX_TOKEN) { r.too_long = true; break; }
        const size_t L = line_len(p, nl);
        r.n_lines++;
        if (L == 0) { r.stopped = true; break; }                    // sketch.go:103-105: break
        if (p[0] == '>') r.hdr_at.push_back((uint64_t)(out - r.buf->as<uint8_t>()));
        else { memcpy(out, p, L); out += L; }
        p = nl + 1;
    }
    r.nbytes = (size_t)(out - r.buf->as<uint8_t>());
}
bool Parser::fasta_block(const Block &blk) {
    if (fa_stopped) return true;
    const uint8_t *base = blk.buf.data(), *end = base + blk.len;
    const uint32_t P = (uint32_t)std::min<size_t>(threads, std::max<size_t>(1, blk.len / 65536));
    std::vector<const uint8_t *> cutp(P + 1);
    cutp[0] = base; cutp[P] = end;
    for (uint32_t i = 1; i < P; i++) {
        const uint8_t *q = base + blk.len * i / P;
        if (q < cutp[i - 1]) q = cutp[i - 1];
        const uint8_t *nl = q < end ? (const uint8_t *)memchr(q, '\n', (size_t)(end - q)) : nullptr;
        cutp[i] = nl ? nl + 1 : end;
    }
    if (fa_pieces.size() < P) fa_pieces.resize(P);
    std::vector<FaPiece> &pc = fa_pieces;
    run_parallel(P, [&](uint32_t i) { fasta_piece(cutp[i], cutp[i + 1], pc[i]); });
    // pieces count up to the first event in stream order
    uint32_t used = P; bool stop = false, too_long = false;
    std::vector<size_t> at(P + 1, 0);
    for (uint32_t i = 0; i < P; i++) {
        at[i + 1] = at[i] + pc[i].nbytes;
        n_lines += pc[i].n_lines;
        if (pc[i].stopped || pc[i].too_long) { used = i + 1; stop = pc[i].stopped; too_long = pc[i].too_long; break; }
    }
    const size_t old = fa_bases.size(), add = at[used];
    uint8_t *dst = fa_bases.grow(add);
    run_parallel(used, [&](uint32_t i) { if (pc[i].nbytes) memcpy(dst + at[i], pc[i].buf->as<uint8_t>(), pc[i].nbytes); });
    // the headers, in stream order: a header closes the record in progress (or, the first one, drops what stood in front of it)
    size_t rec_start = old - fa_cur;                                // where the record in progress begins
    for (uint32_t i = 0; i < used; i++)
        for (const uint64_t h : pc[i].hdr_at) {
            const size_t g = old + at[i] + (size_t)h;               // the header stood in front of byte g
            if (fa_have_hdr) fa_lens.push_back((uint64_t)(g - rec_start));   // store the current entry
            rec_start = g;
            fa_have_hdr = true;
        }
    if (!fa_have_hdr) { fa_bases.n = 0; rec_start = 0; }             // sequence lines before any header are dropped (l2 = nil)
    fa_cur = fa_bases.size() - rec_start;
    // bytes in front of the FIRST header of the stream (no record yet owns them) go
    {
        uint64_t owned = fa_cur;
        for (const uint64_t L : fa_lens) owned += L;
        if (fa_bases.size() > owned) fa_bases.erase_front(fa_bases.size() - (size_t)owned);
    }
    if (too_long) return err.set(HULK_ERR_LINE_TOO_LONG, hulk_strerror(HULK_ERR_LINE_TOO_LONG));
    if (stop) { fa_stopped = true; return true; }
    if (blk.tail_too_long) return err.set(HULK_ERR_LINE_TOO_LONG, hulk_strerror(HULK_ERR_LINE_TOO_LONG));
    if (fa_bases.size() - fa_cur >= FASTA_BATCH_BYTES && !fasta_flush_batch(false)) return false;
    return true;
}
bool Parser::fasta_end() {
    // sketch.go:126-135 flushes the final entry unconditionally; with no header line at all the
    // reference dies on l1[0] = 64 (nil slice) — reported as an error here
    if (!fa_have_hdr) return err.set(HULK_ERR_FASTA_HEADER, hulk_strerror(HULK_ERR_FASTA_HEADER));
    fa_lens.push_back(fa_cur);
    fa_cur = 0;
    return fasta_flush_batch(true);
}

int run_ingest(const char *const *paths, uint32_t n_paths, int fasta, const IngestCfg &cfg, Sink &sink, PhaseTrace &g_trace,
               hulk_ingest_stats *stats, IngestError &err) {
    const auto t0 = std::chrono::steady_clock::now();
    if (n_paths && !paths) { err.set(HULK_ERR_ARG, "NULL path list"); return err.code; }
    uint32_t threads = cfg.parser_threads;
    if (threads == 0) threads = default_parser_threads();       // (a caller's figure is taken as it is)
    if (threads > 256) threads = 256;
    bool ok = true;
    double t_body_end = 0.0;
    {
        BlockReader reader(paths, n_paths, cfg);
        Parser ps(sink, threads, err);
        for (;;) {
            const double tb0 = PhaseTrace::now();
            std::unique_ptr<Block> b = reader.next(err);
            const double tb1 = PhaseTrace::now(); g_trace.wait_block += tb1 - tb0;
            if (!b) { ok = err.code == HULK_OK; break; }
            ok = fasta ? ps.fasta_block(*b) : ps.fastq_block(*b);
            g_trace.parse += PhaseTrace::now() - tb1;
            reader.recycle(std::move(b));
            if (!ok || (fasta && ps.fa_stopped)) break;
        }
        if (ok && fasta) ok = ps.fasta_end();
        if (ok) ok = sink.finish(err);
        if (stats) {
            stats->n_seqs = sink.n_seqs; stats->total_len = sink.total_len; stats->n_lines = ps.n_lines;
            stats->bytes_in = reader.bytes_in();
            stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        t_body_end = PhaseTrace::now();
    }                                                             // (the reader's thread and blocks, the parser's team and buffers go here)
    if (cfg.trace)
        fprintf(stderr, "ingest trace (calling thread, s): next block %.3f | parse + sink %.3f, of which: staging set (wait / first "
                        "allocation) %.3f, copies queued %.3f, hulk_add_reads_device %.3f | releasing the reader and the parser %.3f\n", g_trace.wait_block, g_trace.parse,
                g_trace.stage_wait, g_trace.enqueue, g_trace.add_reads, PhaseTrace::now() - t_body_end);
    return ok ? HULK_OK : err.code;
}

}  // namespace ingest
}  // namespace hulk

using namespace hulk::ingest;

extern "C" {

int hulk_parse_files_opts(const char *const *paths, uint32_t n_paths, int fasta, const hulk_ingest_opts *opts, hulk_batch_fn fn,
                          void *user, hulk_ingest_stats *stats, char *errbuf, uint64_t errbuf_len) {
    IngestError err;
    int rc;
    if (const std::string bad = check_opts(opts); !bad.empty()) {
        err.set(HULK_ERR_ARG, bad); rc = err.code;
    } else {
        CallbackSink sink(fn, user);
        PhaseTrace trace;
        rc = run_ingest(paths, n_paths, fasta, resolve_cfg(opts, 0), sink, trace, stats, err);
    }
    if (errbuf && errbuf_len) {
        const std::string &m = rc == HULK_OK ? std::string() : err.msg;
        const size_t n = std::min<size_t>(m.size(), (size_t)errbuf_len - 1);
        memcpy(errbuf, m.data(), n); errbuf[n] = 0;
    }
    return rc;
}

int hulk_parse_files(const char *const *paths, uint32_t n_paths, int fasta, uint32_t threads, hulk_batch_fn fn,
                     void *user, hulk_ingest_stats *stats, char *errbuf, uint64_t errbuf_len) {
    hulk_ingest_opts o; memset(&o, 0, sizeof o);
    o.parser_threads = threads;
    return hulk_parse_files_opts(paths, n_paths, fasta, threads ? &o : nullptr, fn, user, stats, errbuf, errbuf_len);
}

}  // extern "C"
