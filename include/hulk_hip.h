/*
 * hulk_hip.h — C ABI of libhulkhip.so: the MI355X (gfx950) implementation of HULK's
 * `sketch` hot path (minimizers -> jump-hash k-mer spectrum -> count-min + CWS histosketch).
 *
 * The reference (will-rowe/hulk v1.0.0) has no FFI layer; the seam this library replaces is
 * the Go package API that `SeqMinimizer.Run` / `Sketcher.Run` drive:
 *
 *   reference interface (file:line)                               this ABI
 *   -----------------------------------------------------------   -------------------------
 *   pipeline.findMinimizers(chan, *Info) (*theBoss, error)        hulk_create
 *       src/pipeline/boss.go:54
 *   histosketch.NewHistoSketch(k, s, bins, decay)                 hulk_create (same checks,
 *       src/histosketch/histosketch.go:50-92                        same error strings)
 *   theBoss.AddSeq(seq []byte)        src/pipeline/boss.go:24-26  hulk_add_reads[_device]
 *   theBoss.Flush()                   src/pipeline/boss.go:34-36  hulk_flush
 *   theBoss.StopWork() + final flush  src/pipeline/boss.go:29-31, hulk_finish
 *       src/pipeline/sketch.go:219-224
 *   theBoss.GetMinimizerCount()       src/pipeline/boss.go:39-41  hulk_get_counters
 *   HistoSketch.AddElement(bin, v)    src/histosketch/histosketch.go:129-155
 *                                       (driven internally by hulk_flush; exposed for
 *                                        tests as hulk_add_histogram)
 *   HistoSketch.Sketch / .SketchWeights (exported fields)         hulk_get_sketch
 *       src/histosketch/histosketch.go:40-41
 *   KmerSpectrum bins                 src/kmerspectrum/kmerspectrum.go:25
 *                                                                 hulk_get_histogram
 *   interval rule `seqCount % Interval == 0`                      params.interval
 *       src/pipeline/sketch.go:211-215
 *   DataStreamer.Run + FastqHandler.Run (lines -> reads)          hulk_parse_files (host only),
 *       src/pipeline/sketch.go:40-79, 99-161; seqio.go:38-40        hulk_sketch_files (+ the AddSeq
 *                                                                   loop of sketch.go:196-217)
 *   SeqMinimizer.Run's AddSeq / Flush loop when the read stream   hulk_comm_init + hulk_step_sharded
 *       is sharded over several GPUs                                (+ hulk_gather_sketch for
 *       src/pipeline/sketch.go:182-250, boss.go:24-41               Sketcher.Run's result, sketch.go:271-301)
 *   minhash.KMVsketch.AddHash         src/minhash/kmv.go:39-71     HULK_FLAG_KMV (fed by hulk_add_reads* and every
 *   minhash.KHFsketch.AddHash         src/minhash/khf.go:34-45     HULK_FLAG_KHF  other entry point that bins reads)
 *   MinHash.Merge                     src/minhash/khf.go:49-55     hulk_minhash_merge
 *   theBoss.CollectKMVsketch /        src/pipeline/boss.go:44-51   hulk_get_minhash
 *       CollectKHFsketch                (the reference constructs both sketches, boss.go:70-71, and never feeds them:
 *                                        "not used yet", boss.go:18-19 — feeding them is this library's addition, opt-in)
 *
 * Conventions: every call returns HULK_OK (0) or a negative HULK_ERR_*; the message the
 * reference would have passed to log.Fatalf("ERROR---> %v") is available from
 * hulk_last_error()/hulk_strerror().  The library never aborts the process.  A context is
 * single-caller (the reference's SeqMinimizer.Run is one goroutine).  Caller owns every
 * buffer it passes; host buffers may be released as soon as the call returns.  Work is
 * asynchronous on one HIP stream; hulk_finish / hulk_synchronize / hulk_get_* are the synchronisation points and
 * the place where device-side errors (short read, <1% bins used) surface.
 */
#ifndef HULK_HIP_H
#define HULK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: hulk_params.reserved[0] became `flags` (unknown bits are refused), hulk_set_profiling takes a mask, the multi-GPU
 * entry points (hulk_comm_*, hulk_step_*, hulk_gather_sketch).
 * 3: every knob a host may want per context is a field (as SketchCmd carries every flag as a field,
 *    src/pipeline/pipeline.go:14-30): hulk_params.batch / work_lanes / host_copy_threads (were reserved[0..2], 0 = default),
 *    HULK_FLAG_SHARD_FULL / HULK_FLAG_NO_OVERLAP, hulk_ingest_opts with hulk_parse_files_opts / hulk_sketch_files_opts.
 *    The HULK_* environment variables that remain are overrides for profiling scripts, read when a context is created.
 * 4: HULK_FLAG_CMS_CHAIN + hulk_get_device_checks (the count-min replay's hardware assumption is verified on the device by
 *    hulk_create), hulk_get_profile_table (hulk_set_profiling bit 32), hulk_load_sketches / hulk_smash_files (the directory form
 *    of `hulk smash`); the test hooks hulk_debug_inject / hulk_debug_read left the shipping library (profiling build only).
 *    Additions since (no existing entry point changed): HULK_FLAG_KMV / HULK_FLAG_KHF with hulk_get_minhash / hulk_minhash_merge;
 *    sketch snapshots (hulk_set_snapshots, hulk_snapshot_count, hulk_get_snapshots, hulk_set_snapshot_callback, hulk_poll_snapshots);
 *    a panel the snapshots are scored against (hulk_set_panel, hulk_get_snapshot_distances, hulk_set_snapshot_panel_callback,
 *    hulk_panel_distances); the nearest-neighbour search (hulk_search, hulk_search_files); single-linkage clustering (hulk_cluster,
 *    hulk_cluster_files) and its dendrogram (hulk_dendrogram, hulk_dendrogram_files); complete- and average-linkage dendrograms
 *    (hulk_linkage, hulk_linkage_files).
 * Bindings compare it with the value they were written for. */
#define HULK_ABI_VERSION 4

#define HULK_OK 0
#define HULK_ERR_W (-1)          /* "w must be: 0 < w < 257"                  minimizer.go:63 */
#define HULK_ERR_K (-2)          /* "k size must be: 0 < k < 32"              minimizer.go:66 */
#define HULK_ERR_EMPTY_SEQ (-3)  /* "sequence length must be > 0"             minimizer.go:72 */
#define HULK_ERR_SHORT_SEQ (-4)  /* "sequence length must be >= w + k - 1"    minimizer.go:75 */
#define HULK_ERR_FEW_BINS (-5)   /* "not used yet"                            kmerspectrum.go:95 */
#define HULK_ERR_HS_K (-6)       /* "histosketching only supports k <= 31"    histosketch.go:54 */
#define HULK_ERR_DECAY (-7)      /* "decay ratio must be between 0.0 and 1.0" histosketch.go:63 */
#define HULK_ERR_BINS (-8)       /* "histogram must have at least 2 bins"     histosketch.go:66 */
#define HULK_ERR_NEG_BINS (-9)   /* "negative value used for number of k-mer spectrum bins: %d" kmerspectrum.go:34 */
#define HULK_ERR_NO_SEQ (-10)    /* "no sequences received"                   pipeline/sketch.go:238 */
#define HULK_ERR_FASTQ_ID (-11)  /* "read ID in fastq file does not begin with @: %v"  seqio.go:39 */
#define HULK_ERR_LINE_TOO_LONG (-12) /* "bufio.Scanner: token too long" (a line of >= 64 KiB; sketch.go:53,76 log.Fatal(scanner.Err())) */
#define HULK_ERR_ARG (-30)       /* bad argument to this ABI (NULL pointer, bad shard, ...) */
#define HULK_ERR_HIP (-31)       /* HIP runtime failure; hulk_last_error has the hipError string */
#define HULK_ERR_NO_DEVICE (-32) /* no usable gfx950 device */
#define HULK_ERR_READ_TOO_LONG (-33) /* read longer than this build's per-read limit */
#define HULK_ERR_STATE (-34)     /* call not valid in this state (e.g. add after finish) */
#define HULK_ERR_IO (-35)        /* open/read/gzip failure; the message is the one Go's os/gzip error carries */
#define HULK_ERR_FASTA_HEADER (-36) /* --fasta input without any '>' line (the reference panics on l1[0] = 64, sketch.go:127) */
#define HULK_ERR_COMM (-37)      /* RCCL (or the host's exchange function) failed; hulk_last_error has the detail */

/* How the CWS parameter matrices r, c, b (histosketch.go:95-126) are produced. */
#define HULK_CWS_GO_COMPAT 0     /* go_rng Gamma/Uniform over Go math/rand, seed 1 (default) */
#define HULK_CWS_EXTERNAL 1      /* caller supplies them with hulk_set_cws_tables (e.g. dumped by a Go program) */

/* hulk_params.flags.  None of the NO_* switches changes a result; they only remove an exact shortcut so that
 * its effect can be measured (bench.py --no-prune) and tested (tests/test_gpu_parity.py). */
#define HULK_FLAG_GAMMA_CPYTHON 1u /* go_rng's Gamma (third-party, github.com/leesper/go_rng @ a612b043e353, not vendored by
                                    * the reference: histosketch.go:103,112-113) is restated from memory as CPython's
                                    * gammavariate with the squeeze constant 4*exp(-0.5)/sqrt(2) (the default here); this flag
                                    * selects CPython's own SG_MAGICCONST = 1 + ln 4.5.  Any valid squeeze only short-cuts the
                                    * real test r >= ln z, so the tables are the same either way (tested); the flag exists so
                                    * that a pin against a real Go run can be reproduced literally */
#define HULK_FLAG_NO_PRUNE 2u      /* CWS scan reads the whole table for every interval (no per-tile bound, no whole-batch bound) */
#define HULK_FLAG_NO_SKIP 4u       /* keep the per-tile bound, drop the whole-batch bound */
#define HULK_FLAG_SHARD_FULL 8u    /* hulk_step_sharded always exchanges the k-mer spectra (never the count-min increments) */
#define HULK_FLAG_NO_OVERLAP 16u   /* one stream: flush kernels on the work stream, one work lane (profiling: every kernel
                                    * runs alone, so its own duration can be read) */
#define HULK_FLAG_CMS_CHAIN 64u    /* the count-min replay (countmin.go:103-147 in bin order) runs its chain-form kernels: the order of
                                    * the bins inside a 64-bin chunk comes from a static table and register exchanges instead of from
                                    * the order in which the LDS applies the lanes of one returning atomic add.  hulk_create selects
                                    * them by itself on a device whose LDS does not keep that order (hulk_get_device_checks); same
                                    * additions in the same order: bit-identical counters, estimates and sketch (tested) */
#define HULK_FLAG_NO_PRERESERVE 32u /* hulk_create does not size the work lanes' minimizer lists for batch x interval reads (about
                                     * 3 GB per lane at the defaults): they grow with the first batches instead, at the price of an
                                     * allocation in the middle of the stream.  For contexts that see few or long reads, or many
                                     * contexts (ranks) on one GPU. */

#define HULK_FLAG_KMV 128u         /* feed a bottom-k MinHash with every read's distinct minimizers */
#define HULK_FLAG_KHF 256u         /* feed a k-hash-functions MinHash likewise */
/* With either flag sketch_size must be 1 .. HULK_MINHASH_MAX_SKETCH (HULK_ERR_ARG otherwise; unrestricted without them), and
 * the context holds 3 x sketch_size x 8 bytes + 2 KiB of device memory more (both signatures, a merge staging buffer, counters);
 * a context without the flags allocates none of it and launches the kernels it launched before. */
#define HULK_MINHASH_MAX_SKETCH 4096u

/* Largest k-mer spectrum this build bins: the binning kernels pack (spectrum slot << 20 | bin) into one dword
 * (k^4 = 923,521 < 2^20 at the reference's maximum k = 31; cmd/sketch.go:118). */
#define HULK_MAX_BINS (1 << 20)

typedef struct hulk_ctx hulk_ctx;

typedef struct hulk_params {
    uint32_t k;            /* -k/--kmerSize   (cmd/root.go:62)   */
    uint32_t w;            /* -w/--windowSize (cmd/sketch.go:52) */
    uint32_t sketch_size;  /* -s/--sketchSize (cmd/sketch.go:54) */
    int32_t  num_bins;     /* 0 => Pow(k,4) as cmd/sketch.go:118 */
    double   decay_ratio;  /* -x/--decayRatio (cmd/sketch.go:55); 1.0 = concept drift off */
    uint32_t interval;     /* -i/--interval   (cmd/sketch.go:53); 0 = none */
    int32_t  device;       /* HIP device ordinal */
    uint32_t slot_begin;   /* this context owns sketch slots [slot_begin, slot_begin+slot_count) */
    uint32_t slot_count;   /* 0 => all slots (single-GPU) */
    uint32_t cws_source;   /* HULK_CWS_* */
    uint32_t flags;        /* HULK_FLAG_* (0 = defaults) */
    uint32_t batch;        /* sketching intervals binned by one launch chain and flushed by ONE pass over the CWS table:
                            * 1..16, 0 = default (16).  Any value gives the same sketch (hulk_batch_size) */
    uint32_t work_lanes;   /* 2: consecutive batches are binned on two alternating work streams, so that the minimizer kernel
                            * of a batch runs beside the jump-hash / spectrum kernels of the batch before it; 1: one work
                            * stream; 0 = default: 2, but 1 with count-min decay (0 < decay_ratio < 1), whose flush needs the
                            * CUs a second lane would keep occupied.  A context on a caller's stream (hulk_set_stream) joins the second
                            * lane into that stream at the end of every call — the caller still sees ONE stream — and so
                            * gives up that overlap */
    uint32_t host_copy_threads; /* threads that copy a chunk of hulk_add_reads' host buffers into pinned staging: 1..32,
                            * 0 = default (4) */
    uint32_t reserved;     /* must be 0 */
} hulk_params;

/* Version of this ABI (HULK_ABI_VERSION). */
int hulk_abi_version(void);
/* "abi=4 arch=gfx950 sources=<first 16 hex digits of the SHA-256 over hulk_amd/csrc's sources and headers, in the Makefile's
 * order> hipcc=<version>[ experiments=1]": which tree and compiler this .so was built from (a binding or a test can refuse a
 * stale one); " experiments=1" marks the profiling build (make EXPERIMENTS=1: experiment switches and test hooks compiled in). */
const char *hulk_build_info(void);
/* Reference error text for a status code. */
const char *hulk_strerror(int status);
/* Message of the last failure on this context ("" if none). NULL ctx => last hulk_create failure. */
const char *hulk_last_error(const hulk_ctx *ctx);

/* findMinimizers + NewHistoSketch.  Allocates device state, generates/uploads the CWS tables.  With an interval, the work
 * lanes' buffers are sized here for the largest batch the interval rule forms (batch x interval reads, ~3 GB per lane at
 * the defaults): no call of the stream allocates device memory.  (interval = 0: the first call sizes them.) */
int hulk_create(const hulk_params *params, hulk_ctx **out);
void hulk_destroy(hulk_ctx *ctx);

/* Run all work on the caller's hipStream_t (e.g. torch's current stream) instead of the
 * context's own stream.  NULL is the HIP null (default) stream. */
int hulk_set_stream(hulk_ctx *ctx, void *hip_stream);
/* Go back to the context's private non-blocking stream (the default after hulk_create). */
int hulk_set_private_stream(hulk_ctx *ctx);

/* Supply r, c, b ([sketch_size][num_bins] row-major fp64, full matrices, host memory) when
 * cws_source == HULK_CWS_EXTERNAL.  Must be called before the first read.
 * Domain: K = c * exp(b - r) must be finite in fp32 (|K| <= FLT_MAX, no NaN) for every entry of the rows the context
 * owns — the flush screens candidates with K in fp32; HULK_ERR_ARG otherwise.  newCWS's own tables have |K| < |c|.
 * The check is one exp per entry on the host, single-threaded: sketch_size * num_bins of them, i.e. seconds at
 * sketch_size 1024 and k = 31 (1e9 entries), next to the upload of the same 24 GB. */
int hulk_set_cws_tables(hulk_ctx *ctx, const double *r, const double *c, const double *b);

/* AddSeq for a batch.  Read i is bases[offsets[i] .. offsets[i+1]) (ASCII, any case).
 * The interval rule is applied inside: a flush is queued whenever the global read count hits a
 * multiple of params.interval.  The host variant validates the lengths and has copied the caller's
 * buffers (into pinned staging, in chunks) when it returns — they may be reused at once (the cgo rule);
 * the PCIe copies and the kernels are queued on the context's stream and may still be running:
 * hulk_flush / hulk_finish / the getters are the synchronisation points. */
int hulk_add_reads(hulk_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads);
/* Same, buffers already resident in this device's memory (offsets too).  `max_read_len` is an
 * upper bound on the read lengths in the batch (selects the kernel configuration);
 * `bases_bytes` is the size of the bases allocation.  Length validation happens on device.
 * Stream order: the kernels run on the context's stream (private and non-blocking unless
 * hulk_set_stream was called), so the buffers must be complete before the call — produce them on
 * that stream or synchronise first — and must stay alive until the stream has passed the call. */
int hulk_add_reads_device(hulk_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets,
                          uint64_t n_reads, uint32_t max_read_len, uint64_t bases_bytes);

/* ---- host ingest: DataStreamer.Run + FastqHandler.Run ------------------------
 * Inputs are read in order (n_paths == 0: STDIN; a name whose last '.'-separated element is "gz" is
 * gunzipped), cut into lines the way bufio.Scanner/ScanLines does ('\n', one trailing '\r' dropped,
 * unterminated last line kept, a line of >= 65536 bytes is HULK_ERR_LINE_TOO_LONG) and grouped into
 * reads by the reference's slot machine: FASTQ = l1..l3 take the next NON-EMPTY line, l4 takes the
 * next line whatever it is, the read is l2 and its l1 must start with '@' (checked when l4 arrives,
 * so a truncated last record is dropped silently); --fasta = lines of a '>' record concatenated,
 * parsing stops at the first empty line.  `threads` parser threads (0 = one per core, at most 16; see hulk_ingest_opts).
 * gzip input is inflated by the library itself, multistream as compress/gzip reads it: a regular one-member file of >= 4 MiB
 * by hulk_ingest_opts.gz_threads (default 16) threads at once (about 0.6 GB of scratch mappings while the file is open;
 * HULK_INGEST_GZ_ONE_THREAD: one thread), a bgzip'd file member by member on as many; bytes and messages are the same whichever reader runs. */
typedef struct hulk_ingest_stats {
    uint64_t n_seqs;      /* seqCount of SeqMinimizer.Run */
    uint64_t total_len;   /* lengthTotal */
    uint64_t n_lines;
    uint64_t bytes_in;    /* bytes read (after gunzip) */
    double   seconds;
} hulk_ingest_stats;
/* Called once per parsed batch, in input order; buffers are only valid during the call. */
typedef int (*hulk_batch_fn)(void *user, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads);
/* Parse only (no GPU, no context): every batch goes to `fn`.  Error text -> errbuf. */
int hulk_parse_files(const char *const *paths, uint32_t n_paths, int fasta, uint32_t threads,
                     hulk_batch_fn fn, void *user, hulk_ingest_stats *stats, char *errbuf, uint64_t errbuf_len);
/* The knobs of a run of the host ingest, as fields (0 = the default everywhere).  hulk_parse_files / hulk_sketch_files take
 * the defaults (and `threads` as parser_threads); the HULK_INGEST_* / HULK_GZ_* environment variables, where set, override
 * either — they exist for profiling scripts and tests. */
#define HULK_INGEST_GZ_ONE_THREAD 1u  /* every gzip input through the one-thread reader (no parallel member / BGZF readers) */
#define HULK_INGEST_GZ_ZLIB 2u        /* zlib's inflate instead of the library's own decoder */
#define HULK_INGEST_TRACE 4u          /* seconds per phase of the calling thread and of the gzip readers, on stderr */
#define HULK_INGEST_HOST_PARSER 8u    /* hulk_sketch_files*: lines -> sequences on the host's parser threads.  Default: the raw file
                                       * bytes go to the GPU as they are read and the line machine runs there (hulk_fastq.hip).  FASTQ: a
                                       * block the device will not decide — a header without '@', a line of 64 KiB, an over-long run of
                                       * empty lines — hands the stream to the host parser, whose reads and messages are the same.
                                       * --fasta: the device decides everything (the empty line that ends the parsing, the line of 64 KiB
                                       * that is bufio.Scanner's error); sequences of any length accumulate in device memory across blocks */
#define HULK_INGEST_DEVICE_INFLATE 16u /* hulk_sketch_files* on the device parsers: a regular file whose first member is BGZF (bgzip,
                                       * htslib) has its members inflated on the GPU and the text goes device-to-device to the parser;
                                       * the host only read()s the compressed bytes.  At the first member that is not a clean, verified
                                       * BGZF member the text in front of it is delivered and the file is handed to the one-thread
                                       * host reader at that member, so reads, counters and messages are those of the host path.  STDIN,
                                       * pipes, one-member .gz and plain files are read as without the flag; HULK_INGEST_GZ_ZLIB takes
                                       * precedence.  Accepted and ignored with HULK_INGEST_HOST_PARSER and by hulk_parse_files*.  The
                                       * environment variable HULK_GZ_DEVICE=1 (0) switches it on (off) for any run. */
typedef struct hulk_ingest_opts {
    uint32_t parser_threads;  /* 0 = one per hardware thread, at most 16 (the measured optimum); any other figure is taken as it is (<= 256) */
    uint32_t gz_threads;      /* threads inflating the members of a bgzip'd input, or the chunks of ONE gzip member, side by side: 1..64, 0 = 16 */
    uint32_t file_readers;    /* pieces a block of a regular file is read in, side by side: 1..16, 0 = 4 */
    uint32_t flags;           /* HULK_INGEST_* */
    uint64_t block_bytes;     /* bytes per block of the line pump: >= 128 KiB, 0 = 32 MiB */
    uint64_t gz_chunk_bytes;  /* compressed bytes per chunk of the parallel one-member reader: >= 8 KiB, 0 = 1 MiB */
    uint64_t reserved[2];     /* must be 0 */
} hulk_ingest_opts;
int hulk_parse_files_opts(const char *const *paths, uint32_t n_paths, int fasta, const hulk_ingest_opts *opts,
                          hulk_batch_fn fn, void *user, hulk_ingest_stats *stats, char *errbuf, uint64_t errbuf_len);
/* Parse and AddSeq every read (pinned double-buffered staging, copies and kernels asynchronous on
 * the context's stream while the next block is read and parsed).  The interval rule applies as in
 * hulk_add_reads; the caller still ends the run with hulk_finish (Flush + StopWork). */
int hulk_sketch_files(hulk_ctx *ctx, const char *const *paths, uint32_t n_paths, int fasta, uint32_t threads,
                      hulk_ingest_stats *stats);
int hulk_sketch_files_opts(hulk_ctx *ctx, const char *const *paths, uint32_t n_paths, int fasta, const hulk_ingest_opts *opts,
                           hulk_ingest_stats *stats);
/* The device BGZF inflater on its own: `in` holds whole BGZF members (in_len bytes, nothing else), inflated on the current
 * device into `out`.  *out_len = the text's size (the ISIZE fields summed), *n_members = members framed, *bad_member = index of
 * the first member that failed (UINT64_MAX if none).  out == NULL: a size query (framing only).  Errors: HULK_ERR_IO with
 * "bgzf: member <i> (byte <offset>): <reason>" in errbuf — a piece that is not a whole BGZF member, or a member that fails to
 * inflate (invalid block type, invalid or over-subscribed Huffman code, invalid symbol, distance before the member's start,
 * output longer or shorter than ISIZE, payload exhausted, deflate end not at the payload end, CRC-32 mismatch); HULK_ERR_ARG
 * (out_cap below *out_len), HULK_ERR_HIP.  `out` then holds the text of the members in front of the bad one. */
int hulk_bgzf_inflate(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *n_members,
                      uint64_t *bad_member, char *errbuf, uint64_t errbuf_len);

/* Intervals are flushed in batches: up to hulk_batch_size() consecutive sketching intervals are
 * binned into separate k-mer spectra by one kernel launch and then pushed through count-min + CWS
 * with ONE pass over the CWS table.  The result is identical to flushing them one at a time. */
uint32_t hulk_batch_size(const hulk_ctx *ctx);

/* Multi-GPU split: (1) bin this rank's reads WITHOUT applying the interval rule: read i goes to
 * spectrum i / reads_per_spectrum (0 => all into spectrum 0; at most hulk_batch_size() spectra),
 * (2) the caller all-reduces hulk_histogram_device() across ranks (RCCL, uint32 sum,
 * n_spectra * num_bins contiguous elements), (3) hulk_flush_batch(n_spectra) on every rank. */
int hulk_bin_reads_device(hulk_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets,
                          uint64_t n_reads, uint32_t max_read_len, uint64_t bases_bytes,
                          uint64_t reads_per_spectrum);
/* The same with the first read going to spectrum `first_spectrum` instead of 0 (needs reads_per_spectrum > 0): a rank
 * that bins WHOLE intervals of a batch — intervals [first_spectrum, first_spectrum + n_reads / reads_per_spectrum) —
 * while the other ranks bin the others; the all-reduce over the ring then is a gather (the other spectra are zero here). */
int hulk_bin_reads_device_at(hulk_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets,
                             uint64_t n_reads, uint32_t max_read_len, uint64_t bases_bytes,
                             uint64_t reads_per_spectrum, uint32_t first_spectrum);
/* Spectrum 0 of the batch being binned: hulk_batch_size() spectra of num_bins uint32, contiguous.  The context keeps two
 * such rings and every hulk_flush_batch[_after] (n_spectra > 0) moves on to the other one, so the pointer takes exactly
 * two values, alternating from batch to batch: query it again after every hulk_flush_batch[_after].  Stream order: on a
 * caller's stream (hulk_set_stream) the spectra are complete where that stream has passed hulk_bin_reads_device[_at], and
 * what the caller queues on that stream before hulk_flush_batch — a copy out of the spectra, an all-reduce into them — is
 * passed before the flush reads and wipes them.  A context on its private stream has no such stream to offer: synchronise
 * (hulk_synchronize) before touching the spectra, and hand the stream that touched them to hulk_flush_batch_after. */
uint32_t *hulk_histogram_device(hulk_ctx *ctx);
int hulk_flush_batch(hulk_ctx *ctx, uint32_t n_spectra);
/* Same, but the flush waits for the work queued so far on `dep_stream` (the stream the all-reduce
 * was issued on) instead of the context's work stream, so the next hulk_bin_reads_device on the
 * work stream runs UNDER the collective.  The caller must have made dep_stream wait for the binning
 * (event / wait_stream) before the collective. */
int hulk_flush_batch_after(hulk_ctx *ctx, uint32_t n_spectra, void *dep_stream);

/* ---- multi-GPU with the exchange INSIDE the library (one context = one rank = one GPU) -------------------------
 * The seam is still SeqMinimizer.Run (src/pipeline/sketch.go:182-250) driving theBoss (boss.go:24-41): a host that
 * shards the read stream over G processes calls hulk_comm_init once and then hulk_step_sharded instead of
 * hulk_add_reads_device; the interval rule stays the reference's (a flush every `interval` reads of the GLOBAL stream,
 * sketch.go:211-215) and the sketch is the one a single GPU computes over the same stream.
 *
 * Step s of a G-rank run covers the global sketching intervals [s*G*T, (s+1)*G*T), T = hulk_batch_size(); rank g owns
 * the WHOLE intervals [s*G*T + g*T, s*G*T + (g+1)*T) — one contiguous chunk of T*interval reads — and the sketch
 * slots [slot_begin, slot_begin + slot_count) given at hulk_create (count-min is replicated, the CWS update is
 * slot-sharded).  Per step the library picks one of two exact exchanges on its flush stream:
 *   full   (the first step of a stream, concept drift / decay, or while any rank's whole-step bound says an element
 *           could still lower one of its slots' weights): all-gather of the G*T k-mer spectra, then the ordinary flush
 *           of every rank's T intervals in stream order on every rank;
 *   delta  (steady state: count-min counters only grow and AddElement only replaces a weight by a smaller one,
 *           countmin.go:103-138, histosketch.go:139-153, so once every rank's bound min_row(K)/min(counter) cannot get
 *           below any of its weights, no element can change the sketch): each rank reduces ITS intervals to the
 *           count-min increments they cause (7 x 2000 integers per interval) and their used-bin counts (the 1 % rule,
 *           kmerspectrum.go:84-96), ONE all-gather of those (G*T*56 KB instead of G*T*k^4*4 B), every rank adds them in
 *           stream order.  The bound is evaluated at the start of step s on every rank and travels with step s's
 *           exchange; it governs step s+1 (counters and weights are monotone, so a bound that held one step earlier
 *           still holds).  Integer sums: bit-identical to the full exchange (tested on both paths).
 * The last step of a stream may be ragged: `step_intervals` (the same value on every rank) is the number of intervals
 * of the global stream in this step, rank g holds min(T, max(0, step_intervals - g*T)) of them and the last one may
 * be partial (the reference's EOF flush, sketch.go:219-221).  hulk_finish afterwards only synchronises (and reports
 * "no sequences received", sketch.go:237-239, only if the GLOBAL stream was empty: a rank may hold none of a short stream).
 * Failure: HULK_ERR_ARG / HULK_ERR_STATE are raised before anything is queued and leave the context as it was.  HULK_ERR_HIP /
 * HULK_ERR_COMM from a step are FATAL for the communicator and the run — the peers may be inside a collective this rank has
 * left — and every later call on the context returns the same status; the host ends all ranks. */
#define HULK_UNIQUE_ID_BYTES 128
/* ncclGetUniqueId: called by ONE rank; the host hands the 128 bytes to the other ranks over any channel it has. */
int hulk_comm_unique_id(void *unique_id);
/* ncclCommInitRank (RCCL over xGMI; librccl.so.1 is bound when this is first called).  Collective call. */
int hulk_comm_init(hulk_ctx *ctx, const void *unique_id, uint32_t rank, uint32_t world);
/* The same protocol over a transport the HOST provides (hosts without RCCL between their ranks; the test suite runs two
 * ranks on one GPU this way, which RCCL refuses): the library stages the buffers through pinned host memory and calls
 * `fn` synchronously.  op HULK_XCHG_ALLGATHER: send = this rank's `bytes`, recv = world * bytes, rank order;
 * op HULK_XCHG_ALLREDUCE_U32: element-wise uint32 sum of `bytes` / 4 words over the ranks, send -> recv. */
#define HULK_XCHG_ALLGATHER 0
#define HULK_XCHG_ALLREDUCE_U32 1
typedef int (*hulk_exchange_fn)(void *user, int op, const void *send, void *recv, uint64_t bytes);
int hulk_comm_init_host(hulk_ctx *ctx, uint32_t rank, uint32_t world, hulk_exchange_fn fn, void *user);
/* Projection aid (tools/shard_projection.py): no peer at all — the other ranks' contributions to an all-gather are
 * copies of this rank's own, an all-reduce is the identity.  One GPU then runs exactly one rank's share of a G-rank
 * step, which bounds the G-GPU rate from above. */
int hulk_comm_init_loopback(hulk_ctx *ctx, uint32_t rank, uint32_t world);
/* One step of this rank: bin its whole intervals of the step (n_reads <= T * interval reads, resident in HBM as for
 * hulk_add_reads_device), exchange, flush.  Asynchronous; the next step's binning runs under this step's exchange. */
int hulk_step_sharded(hulk_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                      uint32_t max_read_len, uint64_t bases_bytes, uint32_t step_intervals);
/* The same for reads in HOST memory (a Go host's slices): validated as hulk_add_reads does, copied into pinned staging
 * before the call returns (the cgo rule), PCIe copy and kernels queued on the context's stream. */
int hulk_step_sharded_host(hulk_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint64_t n_reads,
                           uint32_t step_intervals);
/* SURVEY.md 8(e) to the letter, for comparison: every rank bins `reads_per_spectrum` reads of each of `n_spectra`
 * intervals (its slice of every interval), ONE all-reduce (uint32 sum) of the n_spectra spectra, flush. */
int hulk_step_sliced(hulk_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                     uint32_t max_read_len, uint64_t bases_bytes, uint64_t reads_per_spectrum, uint32_t n_spectra);
/* Sketcher.Run's result on every rank (src/pipeline/sketch.go:271-301): all-gather of the ranks' slot shards. */
int hulk_gather_sketch(hulk_ctx *ctx, uint64_t *mins, double *weights);
/* Steps taken by each exchange and the bytes this rank received through the transport (cumulative). */
int hulk_get_comm_stats(hulk_ctx *ctx, uint64_t *steps_delta, uint64_t *steps_full, uint64_t *bytes_received);
/* Health of the exchange headers (cumulative): `refetched` = times this rank's view of a header (its own block in the host
 * transport's staging, or the gathered header of the previous step) was not there when its copy / event said so and was
 * taken again after a synchronisation; `void_blocks` = times a rank's block of the previous step carried another step's seal
 * (every rank then takes the spectra exchange; after a delta step the run ends with HULK_ERR_COMM).  Both are 0 in a healthy run. */
int hulk_get_comm_health(hulk_ctx *ctx, uint64_t *refetched, uint64_t *void_blocks);
/* ---- test hooks: compiled into the PROFILING build only (make -C hulk_amd/csrc EXPERIMENTS=1 -> libhulkhip_exp.so, which
 * defines HULK_EXPERIMENTS; hulk_build_info() then ends in " experiments=1").  The shipping libhulkhip.so does not export them. */
#ifdef HULK_EXPERIMENTS
/* Test hook (tests/test_gpu_two_rank.py): at step `step` of hulk_step_sharded this rank
 *   HULK_INJECT_STALE_SEAL   seals its header block with the PREVIOUS step's tag (a block that is not of this step);
 *   HULK_INJECT_STALE_STAGE  (host transport) finds its own block missing from the host staging on the first attempt. */
#define HULK_INJECT_NONE 0u
#define HULK_INJECT_STALE_SEAL 1u
#define HULK_INJECT_STALE_STAGE 2u
int hulk_debug_inject(hulk_ctx *ctx, uint32_t what, uint64_t step);
/* Test hook: internal buffers of the CWS scan as the latest flush left them (after a synchronisation).
 *   HULK_DEBUG_TILEMIN  float[slot groups][wave tiles][8]: the fp32 tile minima of the batch (no concept drift: plane 0)
 *   HULK_DEBUG_SCANMAP  uint64[slot groups][(wave tiles + 63) / 64]: which tiles the scan read
 *   HULK_DEBUG_NIBBLE   uint32[5 + 17]: the latest short-read binning launch as its work lane holds it (HULK_ERR_STATE before the
 *                       first one; five zeros if that launch binned no reads): spectra of the launch,
 *                       parts per spectrum, bin ranges, log2 of a range's bins, threads of a histogram workgroup (the 4-bit
 *                       kernels, or the exact ones when those ran), then nib_over[17]: which spectra's 4-bit counters overflowed
 * *bytes_io: capacity of `out` in, bytes written out (HULK_ERR_ARG if too small; the size needed is returned in it). */
#define HULK_DEBUG_TILEMIN 1u
#define HULK_DEBUG_SCANMAP 2u
#define HULK_DEBUG_NIBBLE 3u
int hulk_debug_read(hulk_ctx *ctx, uint32_t what, void *out, uint64_t *bytes_io);
#endif /* HULK_EXPERIMENTS */

/* Process-level buffers the library keeps between calls — the device FASTQ parser's pinned and device blocks (hulk_sketch_files:
 * 96 MB pinned and about 300 MB of HBM per set at the default block size; at most two sets, and a set nobody borrowed for 10 s is
 * freed by the process's next hulk_create / hulk_destroy / hulk_sketch_files; a set that has parsed --fasta input also holds a
 * two line indices for 2-byte lines and two accumulation buffers that grow with the longest sequence: about 0.8 GB of HBM more), the
 * host parsers' large buffers (gzip, FASTA, the
 * host FASTQ parser: ordinary memory, at most 1 GiB, same 10 s rule) and hulk_smash's device arrays — are freed at once;
 * the next call that needs them allocates again.  Call it with no hulk_sketch_files / hulk_smash in flight on another thread. */
int hulk_release_caches(void);

/* Test hook: add counts to the current k-mer spectrum directly (host uint32[num_bins]). */
int hulk_add_histogram(hulk_ctx *ctx, const uint32_t *bins);

/* theBoss.Flush(): histosketch the current k-mer spectrum, then wipe it. */
int hulk_flush(hulk_ctx *ctx);
/* Final flush + StopWork; synchronises and reports any deferred device-side error. */
int hulk_finish(hulk_ctx *ctx);

/* Wait until everything queued so far — copies, binning kernels, flushes — has run (the getters below do the same). */
int hulk_synchronize(hulk_ctx *ctx);

/* Outputs (each synchronises the stream).  mins/weights are full length sketch_size; slots not
 * owned by this context keep their initial values (0 / MaxFloat64). */
int hulk_get_sketch(hulk_ctx *ctx, uint64_t *mins, double *weights);
int hulk_get_counters(hulk_ctx *ctx, uint64_t *n_reads, uint64_t *n_minimizers, uint64_t *total_len);
int hulk_get_histogram(hulk_ctx *ctx, uint32_t *bins);
/* ---- the MinHash sketches of `hulk sketch --kmv / --khf` (HULK_FLAG_KMV / HULK_FLAG_KHF) -------------------------------------
 * Both are fed what the boss's collector feeds the k-mer spectrum (boss.go:90-95): for every read, each of its DISTINCT minimizer
 * values hash64(kmer) << 8 | span once — the values hulk_get_counters' n_minimizers counts; a value that occurs in R reads is fed R
 * times.  Interval, decay and slot sharding do not apply; a rank of a sharded run accumulates the MinHash of ITS reads (the host
 * gathers the signatures and merges them).
 *   KMV (kmv.go:39-71): AddHash keeps the sketch_size smallest values of the fed MULTISET (no de-duplication); mins[0 .. *n) ascending,
 *       *n = min(sketch_size, values fed + values merged in).
 *   KHF (khf.go:34-45): mins[i] = min over fed x of (x + i * x) mod 2^64, MaxUint64 while nothing was fed; *n = sketch_size.
 * Order-independent, so bit-exact whatever the batching.  The KHF feed is one min-reduction while 2k + 8 + ceil(log2 sketch_size)
 * <= 64 (no product can wrap: the signature is (i+1) * min(x)); beyond that every value updates every slot (profiles/minhash.txt
 * has the price). */
#define HULK_MINHASH_KMV 0
#define HULK_MINHASH_KHF 1
/* synchronises; mins[sketch_size]; *n = entries held (KMV: min(sketch_size, fed), ascending; KHF: sketch_size);
 * *n_fed = AddHash calls so far (may be NULL).  HULK_ERR_STATE if the context was created without the flag.  Valid on a finished
 * context; on a context with a sticky error it returns that error. */
int hulk_get_minhash(hulk_ctx *ctx, int algo, uint64_t *mins, uint32_t *n, uint64_t *n_fed);
/* MinHash.Merge: fold a signature of the same kind (host array, n entries; KHF needs n == sketch_size, else HULK_ERR_ARG) into the
 * context's: KHF slot-wise minimum (khf.go:49-55), KMV the sketch_size smallest of the two multisets together. */
int hulk_minhash_merge(hulk_ctx *ctx, int algo, const uint64_t *mins, uint32_t n);

/* ---- sketch snapshots: the histosketch after every flushed spectrum, recorded inside the batched flush ---------------------------
 * `hulk sketch --stream` promises "the sketches after every interval" (cmd/sketch.go:56); src/pipeline never reads the flag.  A
 * context with snapshots on records the pair mins[sketch_size] / weights[sketch_size] exactly as hulk_get_sketch would return it
 * right after one flushed spectrum was applied (slots the context does not own: 0 / MaxFloat64) — bit for bit what batch = 1 with
 * hulk_get_sketch after every interval gives, but from inside the batch: the flush kernels walk those states anyway and store
 * them into a device ring of `capacity` snapshots.  Without concept drift such a context scans and resolves per interval (the
 * merged scan keeps one minimum per batch, and the winner of a PREFIX of the batch may sit elsewhere): the first, unpruned
 * batches of a stream pay for that, the steady state (k_flush_decide passes the batch over) costs one small copy kernel per batch.
 * Off by default; a context that never calls hulk_set_snapshots allocates nothing for it and launches what it always did.
 * Not available on the multi-rank paths: on a context with snapshots hulk_bin_reads_device*, hulk_flush_batch*, hulk_comm_init*
 * and hulk_step_* return HULK_ERR_STATE (a delta step of hulk_step_sharded does not run the flush kernels at all).
 * Calling hulk_set_snapshots again (before the first read) starts over: the ring, the callback and a panel set with hulk_set_panel
 * are dropped. */
typedef struct hulk_snapshot_info {
    uint64_t ordinal;   /* 1-based number of the flushed spectrum (interval rule, hulk_flush and hulk_finish's last one alike) */
    uint64_t n_reads;   /* reads of the stream when that spectrum closed */
} hulk_snapshot_info;
/* Before the first read / flush (HULK_ERR_STATE afterwards).  every >= 1: a snapshot after each flushed spectrum whose ordinal is a
 * multiple of `every`; every == 0: off.  hulk_finish's last flush is recorded whatever its ordinal if reads arrived since the last
 * recorded snapshot, and not otherwise (a stream that ends on a recorded interval boundary gets no duplicate); it takes a new
 * ordinal only if reads arrived since the last flush (the empty spectrum behind an interval boundary is not counted).
 * capacity: snapshots the ring holds, 0 = default (64); device and pinned host memory of capacity * sketch_size * 16 bytes each are
 * allocated here, none on the step path.  A flush never records more snapshots than the ring holds: the batch (hulk_batch_size)
 * becomes min(batch, capacity * every) intervals. */
int hulk_set_snapshots(hulk_ctx *ctx, uint32_t every, uint32_t capacity);
/* Host knowledge, no synchronisation: snapshots recorded so far (queued with their flushes), index of the oldest one still held
 * (recorded - capacity once the ring has wrapped).  Either pointer may be NULL. */
int hulk_snapshot_count(hulk_ctx *ctx, uint64_t *recorded, uint64_t *first_held);
/* Synchronises like the other getters.  Copies snapshots [first, first + n) (0-based, in stream order): info[n], mins[n][sketch_size],
 * weights[n][sketch_size] (any of them may be NULL).  A snapshot the ring has dropped or that is not recorded yet: HULK_ERR_ARG. */
int hulk_get_snapshots(hulk_ctx *ctx, uint64_t first, uint32_t n, hulk_snapshot_info *info, uint64_t *mins, double *weights);
/* Delivery without a synchronisation.  fn is called on the caller's thread, in stream order, exactly once per snapshot, from inside
 * hulk_add_reads*, hulk_sketch_files* (between blocks), hulk_flush, hulk_poll_snapshots and hulk_finish, for every recorded snapshot
 * whose flush is found complete (event query, no wait); hulk_finish delivers all that remain.  mins / weights point into the library's
 * pinned staging and are valid during the call only.  With a callback an undelivered snapshot is never overwritten: before a flush
 * that would do so is queued the library waits for the pending ones and delivers them (without a callback the oldest are dropped).
 * A non-zero return of fn ends the run: that call and every later one return HULK_ERR_STATE, "snapshot callback failed".
 * Set it after hulk_set_snapshots and before the first read (HULK_ERR_STATE otherwise). */
typedef int (*hulk_snapshot_fn)(void *user, const hulk_snapshot_info *info, const uint64_t *mins, const double *weights, uint32_t sketch_size);
int hulk_set_snapshot_callback(hulk_ctx *ctx, hulk_snapshot_fn fn, void *user);
/* Hands the snapshots of every flush that has run to the callback; never blocks.  *delivered (may be NULL): how many. */
int hulk_poll_snapshots(hulk_ctx *ctx, uint32_t *delivered);

/* ---- a panel of reference sketches: every snapshot is scored where it is recorded ------------------------------------------------
 * The panel — n_panel histosketches of sketch_size slots, host arrays [n_panel][sketch_size] — is uploaded once and kept on the device
 * slot-major.  Behind the kernels of every flush that records snapshots one more kernel (k_snap_panel) compares the flush's <= 16
 * snapshots with all of it: distances[p] = HULKdata.GetDistance (src/sketchio/sketchio.go:259-306) exactly as hulk_smash computes it —
 * mins compared as float64, jaccard = 1 - equal / sketch_size, weightedjaccard = GetWJD with both weight vectors the SUBJECT's,
 * |w| = max(max(w,0), max(-w,0)), the fp64 sums taken over the slots in ascending order — so a snapshot's distances are bit for bit
 * what `smash` prints for it if its file lay in the panel's directory (a weighted distance that is 0 / 0 or Inf / Inf is the NaN with
 * the sign bit set, 0xFFF8000000000000, which the reference's division gives on amd64; hulk_smash leaves the GPU's unsigned one):
 *   HULK_PANEL_ROW     the snapshot is the subject (its row of that matrix; the snapshot's weights)
 *   HULK_PANEL_COLUMN  each panel sketch is the subject (its column; the panel's weights).  For jaccard the two are the same.
 * The distances go to a device ring [capacity][n_panel] next to the snapshot ring and travel with the snapshots: same indices, same
 * dropping, same delivery; no synchronisation and no allocation on the step path.  A context without a panel allocates none of this
 * and launches what it always did. */
#define HULK_PANEL_ROW 0
#define HULK_PANEL_COLUMN 1
#define HULK_PANEL_MAX 65536u
/* After hulk_set_snapshots and before the first read / flush (HULK_ERR_STATE otherwise).  metric: HULK_METRIC_JACCARD /
 * HULK_METRIC_WEIGHTED_JACCARD.  sketch_size other than the context's: HULK_ERR_ARG, "sketch length mismatch: %d vs %d\n" (the
 * context's, the panel's; sketchio.go:274-277).  n_panel > HULK_PANEL_MAX: HULK_ERR_ARG.  n_panel == 0 removes the panel.  Allocates
 * the panel (n_panel * sketch_size * 16 bytes of device memory) and the distance ring with its pinned mirror (capacity * n_panel * 8
 * bytes each).  A later hulk_set_panel replaces the panel; a later hulk_set_snapshots drops it (the ring it was sized for is gone). */
int hulk_set_panel(hulk_ctx *ctx, const uint64_t *mins, const double *weights, uint32_t n_panel, uint32_t sketch_size, int metric,
                   int role);
/* Synchronises like hulk_get_snapshots and fails like it for a dropped or not yet recorded snapshot: out[n][n_panel], the distances of
 * snapshots [first, first + n).  HULK_ERR_STATE on a context without a panel. */
int hulk_get_snapshot_distances(hulk_ctx *ctx, uint64_t first, uint32_t n, double *out);
/* hulk_set_snapshot_callback's rules (stream order, exactly once, no overwrite of an undelivered snapshot, a non-zero return ends the
 * run), with the snapshot's distances[n_panel] (pinned staging, valid during the call; NULL / 0 without a panel).  A context has ONE
 * callback: setting either kind replaces the other. */
typedef int (*hulk_snapshot_panel_fn)(void *user, const hulk_snapshot_info *info, const uint64_t *mins, const double *weights,
                                      uint32_t sketch_size, const double *distances, uint32_t n_panel);
int hulk_set_snapshot_panel_callback(hulk_ctx *ctx, hulk_snapshot_panel_fn fn, void *user);
/* The same kernel on host arrays, without a context: out[m][n_panel] = the distance of snapshot i (snap_mins / snap_weights
 * [m][sketch_size]) and panel sketch p in the given role; the snapshots are taken 16 at a time.  A one-against-many query. */
int hulk_panel_distances(int device, const uint64_t *snap_mins, const double *snap_weights, uint32_t m, const uint64_t *panel_mins,
                         const double *panel_weights, uint32_t n_panel, uint32_t sketch_size, int metric, int role, double *out);

/* Count-min counters as fp64 [7][2000] (test hook). */
int hulk_get_cms(hulk_ctx *ctx, double *counters);
/* Copy rows of the CWS tables owned by this context to host: each [slot_count][num_bins] (test hook). */
int hulk_get_cws_tables(hulk_ctx *ctx, double *r, double *c, double *b);

/* `hulk smash` (cmd/smash.go:183-226): pairwise distance matrix of n_sketches histosketches of
 * sketch_size slots (host arrays, row-major).  distances[s * n + q] = HULKdata.GetDistance(subject s,
 * query q) (src/sketchio/sketchio.go:259-306): jaccard = distances.go:19-26, weighted jaccard =
 * distances.GetWJD (distances.go:44-72) with the subject's weights on both sides, as the reference does. */
#define HULK_METRIC_JACCARD 0
#define HULK_METRIC_WEIGHTED_JACCARD 1
/* Bottom-k set similarity, the estimator of a KMV sketch (KMVsketch.GetSimilarity, src/minhash/kmv.go:119-159): with the two value
 * lists taken as multisets of uint64 (never through float64), intersect = the sum over the distinct values v of
 * min(multiplicity in A, multiplicity in B), distance = 1.0 - (double)intersect / (double)sketch_size.  Symmetric: no subject, the
 * role of a search is ignored.  The order of a sketch's values does not matter (the device sorts every sketch once); `weights` is
 * never read and may be NULL.  sketch_size at most HULK_MINHASH_MAX_SKETCH.  Both lists have sketch_size values, as everywhere in
 * this interface: lists of unequal length, which GetSimilarity tolerates, are not supported.  Accepted by hulk_smash, hulk_smash_ex,
 * hulk_search, hulk_cluster and hulk_dendrogram, with the same bits for a pair in all of them; not by the panel entry points.
 * (The value 2 is no metric.) */
#define HULK_METRIC_BOTTOMK 3
int hulk_smash(int device, const uint64_t *mins, const double *weights, uint32_t n_sketches,
               uint32_t sketch_size, int metric, double *distances);
/* The same; *kernel_ms (may be NULL) receives the duration of the distance kernel alone (HIP events), without the PCIe copies. */
int hulk_smash_ex(int device, const uint64_t *mins, const double *weights, uint32_t n_sketches,
                  uint32_t sketch_size, int metric, double *distances, double *kernel_ms);

/* What hulk_create verified on this context's device.  *lds_order_ok: 1 if one returning LDS atomic add (ds_add_rtn_u64 /
 * ds_add_rtn_f64) applies the lanes that hit one address in ascending lane order and a wave's instructions in program order —
 * the property the count-min replay kernels take the reference's bin order from (countmin.go:103-138); checked once per
 * process and device with all-equal, paired and pseudo-random address patterns.  *cms_chain_form: 1 if this context runs the
 * chain-form replay kernels (the property does not hold, or HULK_FLAG_CMS_CHAIN). */
int hulk_get_device_checks(hulk_ctx *ctx, uint32_t *lds_order_ok, uint32_t *cms_chain_form);

/* ---- `hulk smash`, the directory form (cmd/smash.go:160-226), native: LoadHULKdata for every file (sketchio.go:100-195: JSON,
 * class / version, the MD5 of the little-endian mins against the stored md5sum, helpers.go:156-166) on `threads` host threads
 * (0 = one per hardware thread, at most 32), FindSketch(ksize, algo) per file (sketchio.go:198-257), the equal-length check of
 * GetDistance (sketchio.go:274-277).  Paths are taken in sort.Strings order (a path given twice counts once: the reference keeps
 * them in a map).  Failures: HULK_ERR_ARG with the reference's text in `errbuf` (and hulk_last_error(NULL)) — of the first file
 * in sorted order that fails to load; then "<n> sketches found ... needs at least 2"; then of the first file whose FindSketch
 * fails; then the length mismatch.  hulk_load_sketches needs no GPU. */
typedef struct hulk_sketch_set hulk_sketch_set;
int hulk_load_sketches(const char *const *paths, uint32_t n_paths, uint32_t ksize, const char *algo, uint32_t threads,
                       hulk_sketch_set **out, char *errbuf, uint64_t errbuf_len);
void hulk_sketch_set_free(hulk_sketch_set *set);
int hulk_sketch_set_info(const hulk_sketch_set *set, uint32_t *n_sketches, uint32_t *sketch_size);
const uint64_t *hulk_sketch_set_mins(const hulk_sketch_set *set);      /* [n_sketches][sketch_size], sorted-path order */
const double *hulk_sketch_set_weights(const hulk_sketch_set *set);     /* the same shape (zeros for kmv / khf: they carry no weights) */
const char *hulk_sketch_set_path(const hulk_sketch_set *set, uint32_t i);
const char *hulk_sketch_set_banner(const hulk_sketch_set *set, uint32_t i);   /* banner_label of file i */
typedef struct hulk_smash_stats {
    double seconds_load;     /* reading, parsing and verifying the files */
    double seconds_matrix;   /* hulk_smash (copies + kernels) */
    double seconds_csv;      /* formatting and writing the CSV file(s) */
    double kernel_ms;        /* the distance kernel alone */
    uint32_t n_sketches, sketch_size;
} hulk_smash_stats;
/* runSmash + makeMatrix: load, smash on `device`, and — matrix_csv_path != NULL — write the file encoding/csv would: the sorted
 * paths as header, then one row per subject of strconv.FormatFloat(100 - 100 * distance, 'f', 2, 64) (cmd/smash.go:183-226);
 * banner_csv_path != NULL: makeBannerMatrix's file (cmd/smash.go:229-261: a sketch's mins + its banner label per line, in
 * sorted file order).  metric: "jaccard" | "weightedjaccard" | "bottomk" (HULK_METRIC_BOTTOMK; with algo "kmv" only: any other
 * algorithm is HULK_ERR_ARG, "bottomk is only supported for kmv sketches", where "weighted jaccard is only supported for
 * histosketches" is checked; the same in hulk_search_files, hulk_cluster_files and hulk_dendrogram_files); algo: "histosketch" | "kmv" | "khf".  `distances` (may be NULL)
 * receives [n][n] in sorted-path order; `stats` may be NULL. */
int hulk_smash_files(int device, const char *const *paths, uint32_t n_paths, uint32_t ksize, const char *algo, const char *metric,
                     uint32_t threads, const char *matrix_csv_path, const char *banner_csv_path, double *distances,
                     hulk_smash_stats *stats, char *errbuf, uint64_t errbuf_len);

/* ---- nearest-neighbour search: for every query sketch the K closest sketches of a database ----------------------------------------
 * distance(query i, database sketch p) = HULKdata.GetDistance exactly as hulk_smash computes it (mins compared as float64, jaccard =
 * 1 - equal / sketch_size, weightedjaccard = GetWJD with both weight vectors the SUBJECT's, |w|, fp64 sums over the slots in ascending
 * order): bit for bit the entry `smash` prints with both files in one directory.  role as for the panel: HULK_PANEL_ROW the query is
 * the subject (its weights), HULK_PANEL_COLUMN the database sketch is; for jaccard the two are the same.
 * The hit list of query i: the pairs whose distance is not NaN and, if max_distance is in [0, 1], is <= max_distance (a negative
 * value or NaN: no limit), ordered by (distance ascending, database index ascending) — a total order: the result does not depend on
 * scheduling, strip size or launch shape — cut to the first k.  hit_count[i] <= k is its length; hit_index / hit_distance [m][k] hold
 * it, the entries behind hit_count[i] are 0xFFFFFFFF / NaN.  HULK_SEARCH_SELF: the database is the query set itself (db_mins and
 * db_weights NULL, n_db ignored) and the pair (i, i) is left out: the k-nearest-neighbour graph of a collection.
 * The prepared queries stay on the device; the database streams through it strip by strip (upload, prepare, distances of a block of
 * queries x the strip into a scratch, selection into the running lists: k_search_dist, k_search_select in hulk_search.hip), so device
 * memory is the queries plus scratch_bytes whatever n_db is, and no m x n_db array exists anywhere.  scratch_bytes (0 = default,
 * 1 GiB) holds one strip (raw and prepared: 32 * sketch_size bytes per database sketch) and the distances of query block x strip.
 * HULK_ERR_ARG before any HIP call, with a text in hulk_last_error(NULL): NULL arrays; k == 0 or k > HULK_SEARCH_MAX_K; m, n_db or
 * sketch_size == 0; an unknown metric, role or flag; non-zero reserved; HULK_SEARCH_SELF together with db arrays, or no db arrays
 * without it; a scratch_bytes too small for one tile (32 queries x 64 database sketches). */
#define HULK_SEARCH_MAX_K 64u
#define HULK_SEARCH_SELF 1u
typedef struct hulk_search_opts {
    uint32_t k;              /* hits per query, 1 .. HULK_SEARCH_MAX_K */
    int metric;              /* HULK_METRIC_JACCARD / HULK_METRIC_WEIGHTED_JACCARD / HULK_METRIC_BOTTOMK */
    int role;                /* HULK_PANEL_ROW / HULK_PANEL_COLUMN */
    uint32_t flags;          /* HULK_SEARCH_SELF */
    double max_distance;     /* in [0, 1]: only hits with distance <= max_distance; negative or NaN: no limit */
    uint64_t scratch_bytes;  /* 0 = default */
    uint64_t reserved[4];    /* zero */
} hulk_search_opts;
typedef struct hulk_search_stats {
    double seconds_total;    /* the whole call */
    double kernel_ms_dist;   /* k_search_dist, summed over the strips and query blocks (HIP events) */
    double kernel_ms_select; /* k_search_select, the same */
    uint32_t strips, query_blocks;
} hulk_search_stats;
int hulk_search(int device, const uint64_t *q_mins, const double *q_weights, uint32_t m, const uint64_t *db_mins,
                const double *db_weights, uint32_t n_db, uint32_t sketch_size, const hulk_search_opts *opts, uint32_t *hit_index,
                double *hit_distance, uint32_t *hit_count, hulk_search_stats *stats);
/* The directory form: both sets of sketch files go through hulk_load_sketches' loader (MD5, FindSketch, the reference's error texts;
 * sorted path order within each set, a path given twice counts once) — but a set of ONE sketch is valid here: "needs at least 2" is
 * smash's rule.  Different sketch lengths across the sets: "sketch length mismatch: %d vs %d\n" (the queries', the database's).
 * HULK_SEARCH_SELF in flags: db_paths NULL, the queries are searched among themselves.  metric: "jaccard" | "weightedjaccard" | "bottomk" (kmv only); algo:
 * "histosketch" | "kmv" | "khf".  csv_path != NULL: a file with the header "query,rank,hit,similarity" and one line per hit, in query
 * order and then rank order from 1: the two paths as encoding/csv quotes them and strconv.FormatFloat(100 - 100 * distance, 'f', 2, 64),
 * the string `smash` prints for that pair.  hit_index / hit_distance [unique query paths][k] and hit_count may be NULL; the indices
 * count the database's sorted unique paths. */
int hulk_search_files(int device, const char *const *query_paths, uint32_t n_q, const char *const *db_paths, uint32_t n_db,
                      uint32_t ksize, const char *algo, const char *metric, int role, uint32_t k, double max_distance, uint32_t flags,
                      uint32_t threads, const char *csv_path, uint32_t *hit_index, double *hit_distance, uint32_t *hit_count,
                      hulk_search_stats *stats, char *errbuf, uint64_t errbuf_len);

/* ---- single-linkage clustering of a sketch collection at a distance threshold ---------------------------------------------------
 * d(i, j) = entry [i][j] of the matrix hulk_smash gives (sketch i the subject), bit for bit.  Sketches i != j are LINKED when
 * d(i, j) <= max_distance or d(j, i) <= max_distance: the compare is on the double itself, a NaN never links, a distance equal to the
 * threshold does.  (jaccard: both directions are the same bits; weightedjaccard uses the subject's weights on both sides, so they are
 * not, and one direction is enough.)  A cluster is a connected component of that graph; label[i] is the smallest index in i's
 * component — a function of the inputs alone: bands, tiles, scheduling and timing cannot change it.  stats->links: the number of
 * ordered pairs (i, j), i != j, with d(i, j) <= max_distance; stats->clusters: the number of i with label[i] == i.
 * The whole set is prepared once and stays on the device (16 * sketch_size bytes a sketch; with the raw upload the peak is
 * 32 * sketch_size * n bytes; that and HULK_CLUSTER_MAX_N limit n); no n x n array exists.  k_cluster_link (hulk_cluster.hip) is launched once per
 * band of band_rows subject rows, a lock-free union-find keeps the components.
 * HULK_ERR_ARG before any HIP call, with a text in hulk_last_error(NULL): NULL arrays or opts; n or sketch_size == 0; an unknown
 * metric; max_distance outside [0, 1] (NaN included); band_rows not a multiple of 32; non-zero flags or reserved; n above
 * HULK_CLUSTER_MAX_N (the set is prepared in one launch).  n == 1 is valid: one cluster, 0 links. */
#define HULK_CLUSTER_MAX_N 2097088u
typedef struct hulk_cluster_opts {
    int metric;            /* HULK_METRIC_JACCARD / HULK_METRIC_WEIGHTED_JACCARD / HULK_METRIC_BOTTOMK */
    double max_distance;   /* tau in [0, 1]; anything else (NaN included): HULK_ERR_ARG */
    uint32_t band_rows;    /* subject rows per launch; 0 = default (2048, search's block); a multiple of 32 (above 2^20: 2^20) */
    uint32_t flags;        /* zero */
    uint64_t reserved[4];  /* zero */
} hulk_cluster_opts;
typedef struct hulk_cluster_stats {
    double seconds_total, kernel_ms_link, kernel_ms_flatten;   /* the whole call; k_cluster_link / k_cluster_flatten summed over the bands (HIP events) */
    uint64_t links;
    uint32_t bands, clusters;
} hulk_cluster_stats;
int hulk_cluster(int device, const uint64_t *mins, const double *weights, uint32_t n, uint32_t sketch_size,
                 const hulk_cluster_opts *opts, uint32_t *label, hulk_cluster_stats *stats);
/* The directory form: the files go through hulk_load_sketches' loader (MD5, FindSketch, the reference's error texts; sorted unique
 * paths; a set of ONE sketch is valid).  metric: "jaccard" | "weightedjaccard" (histosketches only: hulk_smash_files' text) | "bottomk" (kmv only: likewise); algo:
 * "histosketch" | "kmv" | "khf".  label [unique paths] may be NULL.  csv_path != NULL: a file with the header
 * "sketch,cluster,size,representative" and one line per sketch in sorted path order: its path, the 1-based ordinal of its cluster
 * (clusters ordered by their smallest member), the cluster's member count, the path of its smallest member; paths as encoding/csv
 * quotes them. */
int hulk_cluster_files(int device, const char *const *paths, uint32_t n, uint32_t ksize, const char *algo, const char *metric,
                       double max_distance, uint32_t threads, const char *csv_path, uint32_t *label,
                       hulk_cluster_stats *stats, char *errbuf, uint64_t errbuf_len);

/* ---- the links of a sketch collection as a sparse graph: every pair within a distance, with its distance ----------------------------
 * d(i, j) = entry [i][j] of the matrix hulk_smash gives (sketch i the subject), bit for bit.  Row i of the result lists every j != i
 * with d(i, j) <= max_distance, in ascending j: the compare is on the double itself, equality is in, a NaN never is — hulk_cluster's
 * link rule for ONE direction.  The result is CSR: row_start[n + 1] (uint64), col[edges] (uint32), distance[edges] (double, the very
 * bits hulk_smash gives); edges = row_start[n] is hulk_cluster's stats->links at the same threshold.  weightedjaccard is directed
 * (the subject's weights are used on both sides); jaccard and bottomk come out symmetric.  HULK_LINKS_UPPER: only j > i — for the two
 * symmetric metrics the graph without its mirror image, for weightedjaccard the upper part of the directed graph; the tiles wholly
 * below the diagonal are not computed.  Without it every metric pays the full square, about twice hulk_cluster's triangle for jaccard
 * and bottomk.  A function of the inputs alone: bands, tile shape, scheduling and repeats cannot change a byte; the host sorts nothing.
 * The set is prepared once and stays on the device as in hulk_cluster (the same peak of 32 * sketch_size * n bytes); no n x n array
 * exists on the device or the host.  Per band of band_rows subject rows: k_links_count (hulk_links.hip: hulk_cluster's tile; one 64-bit
 * mask per row and tile of 64 columns), a scan of the masks' popcounts, one synchronisation in which the host reads the band's edge
 * count, and k_links_fill over the tiles that hold an edge, which computes those tiles again and writes every edge to its final
 * slot.  Beside the set the device holds 12.25 bytes per (row of the band, 64 columns) — the band is shrunk, in steps of 32 rows, to
 * fit — and 12 bytes per edge of the densest band.  When everything links the call costs two passes of the tile.
 * The result is an object the library owns (as hulk_sketch_set): the caller cannot know `edges` in advance.
 * HULK_ERR_ARG before any HIP call, with a text in hulk_last_error(NULL): NULL arrays (weights may be NULL for bottomk), opts or out;
 * n or sketch_size == 0; an unknown metric; bottomk above HULK_MINHASH_MAX_SKETCH; max_distance outside [0, 1] (NaN included);
 * band_rows not a multiple of 32; unknown flags; non-zero reserved; n above HULK_CLUSTER_MAX_N.  n == 1 is valid: 0 edges.
 * max_edges != 0 and more edges than that: the call stops behind the first band whose running count crosses the cap and returns
 * HULK_ERR_ARG (the cap is an argument the input does not fit) with a text that names the cap and the count reached, *out = NULL and
 * the count so far in stats->edges (stats->bands: the bands counted).  A band whose edges do not fit in device memory ends the call
 * the same way with HULK_ERR_HIP. */
#define HULK_LINKS_UPPER 1u
typedef struct hulk_links_opts {
    int metric;            /* HULK_METRIC_JACCARD / HULK_METRIC_WEIGHTED_JACCARD / HULK_METRIC_BOTTOMK */
    double max_distance;   /* tau in [0, 1]; anything else (NaN included): HULK_ERR_ARG */
    uint32_t band_rows;    /* subject rows per launch; 0 = default (2048); a multiple of 32 (above 2^20: 2^20) */
    uint32_t flags;        /* HULK_LINKS_UPPER */
    uint64_t max_edges;    /* 0 = no cap other than memory */
    uint64_t reserved[4];  /* zero */
} hulk_links_opts;
typedef struct hulk_links_stats {
    double seconds_total, kernel_ms_count, kernel_ms_fill;   /* the whole call; k_links_count / k_links_fill summed over the bands (HIP events) */
    uint64_t edges;
    uint32_t bands, max_degree;   /* max_degree: the longest row */
} hulk_links_stats;
typedef struct hulk_link_list hulk_link_list;
int hulk_links(int device, const uint64_t *mins, const double *weights, uint32_t n, uint32_t sketch_size,
               const hulk_links_opts *opts, hulk_link_list **out, hulk_links_stats *stats);
int hulk_link_list_info(const hulk_link_list *list, uint32_t *n, uint64_t *edges);   /* HULK_ERR_ARG for NULL; n / edges may be NULL */
const uint64_t *hulk_link_list_row_start(const hulk_link_list *list);   /* [n + 1]; NULL for NULL (the three of them) */
const uint32_t *hulk_link_list_cols(const hulk_link_list *list);        /* [edges] */
const double *hulk_link_list_distances(const hulk_link_list *list);     /* [edges] */
void hulk_link_list_free(hulk_link_list *list);                         /* NULL is fine */
/* The directory form: hulk_cluster_files' loader, error texts and their order, "one sketch is valid", and its weightedjaccard /
 * bottomk algorithm checks.  The rows count the sorted unique paths.  csv_path != NULL: a file with the header
 * "sketch,neighbour,distance,similarity" and one line per edge in CSR order: the two paths as encoding/csv quotes them, the distance
 * as %.17g (it reads back to the same double) and strconv.FormatFloat(100 - 100 * distance, 'f', 2, 64), the string `smash` prints
 * for that pair.  out may be NULL (the list is freed); otherwise *out is the caller's to free. */
int hulk_links_files(int device, const char *const *paths, uint32_t n, uint32_t ksize, const char *algo, const char *metric,
                     double max_distance, uint32_t flags, uint64_t max_edges, uint32_t threads, const char *csv_path,
                     hulk_link_list **out /* may be NULL */, hulk_links_stats *stats, char *errbuf, uint64_t errbuf_len);

/* ---- the single-linkage dendrogram of a sketch collection: every threshold of hulk_cluster at once ---------------------------------
 * d(i, j) = entry [i][j] of the matrix hulk_smash gives (sketch i the subject), bit for bit.  The undirected edge {i, j}, i != j,
 * weighs w(i, j) = fmin(d(i, j), d(j, i)) — a NaN direction is ignored, two NaN directions are no edge: hulk_cluster's "either
 * direction links" for every threshold at once (jaccard: both directions are the same bits; weightedjaccard: they are not).  Edges
 * are totally ordered by the key (w, lo, hi), lo = min(i, j), hi = max(i, j) (w >= 0: a double that orders like its bits), and the
 * result is the minimum spanning forest under that order — what Kruskal gives on the edges sorted by the key; unique however many
 * distances tie.  *n_edges = n - (connected components of the non-NaN graph); edge_a[e] < edge_b[e] and edge_distance[e], n - 1 entries
 * each, receive the edges ascending by the key: the merge order of the dendrogram.  For any tau the components of
 * {e: edge_distance[e] <= tau}, labelled by their smallest member, are hulk_cluster's labels at max_distance = tau.  A function of
 * the inputs alone: bands, launch shape, the number of rounds and scheduling cannot change a bit.  n == 1: 0 edges; every pair NaN
 * (every weight row zero under weightedjaccard): 0 edges, n components, HULK_OK.
 * Boruvka's algorithm: the set is prepared once and stays on the device as in hulk_cluster (the same peak, or the set plus a scratch
 * of 12 * (band_rows * ceil(n / 64) + 64 * ceil(n / 64) * band_rows / 32) bytes); a ROUND is one pass of k_dendro_offer
 * (hulk_dendrogram.hip: hulk_cluster's tile, keeping per sketch the closest sketch of another component) in bands of band_rows
 * subject rows, k_dendro_fold behind every band, and a contraction of the n offers on the host (hulk_boruvka.h).  At most
 * ceil(log2 n) rounds deliver offers; one more, empty, closes a forest that NaNs separate: stats->rounds <= ceil(log2 n) + 1, 0 for
 * n == 1.  No n x n array exists.
 * HULK_ERR_ARG before any HIP call, with a text in hulk_last_error(NULL): NULL arrays, opts or n_edges; n or sketch_size == 0; an
 * unknown metric; band_rows not a multiple of 32; non-zero flags or reserved; n above HULK_CLUSTER_MAX_N. */
typedef struct hulk_dendrogram_opts {
    int metric;            /* HULK_METRIC_JACCARD / HULK_METRIC_WEIGHTED_JACCARD / HULK_METRIC_BOTTOMK */
    uint32_t band_rows;    /* subject rows per launch; 0 = default (2048); a multiple of 32 (above 2^20: 2^20) */
    uint32_t flags;        /* zero */
    uint64_t reserved[4];  /* zero */
} hulk_dendrogram_opts;
typedef struct hulk_dendrogram_stats {
    double seconds_total, kernel_ms_offer, kernel_ms_fold;   /* the whole call; k_dendro_offer / k_dendro_fold summed over rounds and bands (HIP events, read behind each round's one synchronisation) */
    uint32_t rounds, bands /* per round */, edges, components;
} hulk_dendrogram_stats;
int hulk_dendrogram(int device, const uint64_t *mins, const double *weights, uint32_t n, uint32_t sketch_size,
                    const hulk_dendrogram_opts *opts, uint32_t *edge_a, uint32_t *edge_b, double *edge_distance /* n - 1 each */,
                    uint32_t *n_edges, hulk_dendrogram_stats *stats);
/* The directory form: the files go through hulk_load_sketches' loader (MD5, FindSketch, the reference's error texts; sorted unique
 * paths, which the indices count; a set of ONE sketch is valid).  metric: "jaccard" | "weightedjaccard" (histosketches only:
 * hulk_smash_files' text) | "bottomk" (kmv only: likewise); algo: "histosketch" | "kmv" | "khf".  edge_a / edge_b / edge_distance [unique paths - 1] and n_edges may be
 * NULL.  csv_path != NULL: a file with the header "merge,sketch_a,sketch_b,distance,similarity,size" and one line per edge in merge
 * order: the 1-based ordinal, the two paths as encoding/csv quotes them, the distance as %.17g (it reads back to the same double: a
 * cut can be repeated exactly), strconv.FormatFloat(100 - 100 * distance, 'f', 2, 64) as `smash` prints it, and the size of the
 * cluster the merge creates.  cut_distance in [0, 1] and cut_csv_path != NULL: the file hulk_cluster_files writes at max_distance =
 * cut_distance, byte for byte ("sketch,cluster,size,representative"), from the edges with distance <= cut_distance; cut_distance NaN:
 * no cut (cut_csv_path is ignored); any other cut_distance, or one in [0, 1] without a cut_csv_path, is HULK_ERR_ARG. */
int hulk_dendrogram_files(int device, const char *const *paths, uint32_t n, uint32_t ksize, const char *algo, const char *metric,
                          uint32_t threads, const char *csv_path, double cut_distance /* NaN: no cut */, const char *cut_csv_path,
                          uint32_t *edge_a, uint32_t *edge_b, double *edge_distance, uint32_t *n_edges,
                          hulk_dendrogram_stats *stats, char *errbuf, uint64_t errbuf_len);

/* ---- single-, complete- and average-linkage dendrograms of a sketch collection -----------------------------------------------------
 * D = the matrix hulk_smash gives for the set, bit for bit; W[i][j] = fmin(D[i][j], D[j][i]) for i != j, as in hulk_dendrogram; a pair
 * whose two directions are NaN has W = +inf and never merges.  Clusters start as the n singletons and are named by their smallest
 * member.  While some pair of live clusters is at a finite distance, the pair (p, q), p < q, that is smallest under the key
 * (d(p, q), p, q) merges: merge t = (p, q, d(p, q), size_p + size_q), the union keeps the name p, and for every other live k
 *   HULK_LINKAGE_SINGLE    d(p, k) = min(d(p, k), d(q, k))
 *   HULK_LINKAGE_COMPLETE  d(p, k) = max(d(p, k), d(q, k))
 *   HULK_LINKAGE_AVERAGE   d(p, k) = (n_p * d(p, k) + n_q * d(q, k)) / (n_p + n_q): n_p, n_q the sizes before the merge as doubles,
 *                          each of the two products, the sum and the quotient rounded on its own (no fused multiply-add); +inf propagates
 * *n_merges = n - (the clusters left when no finite pair remains): under single linkage the connected components of the finite graph;
 * under complete and average linkage +inf propagates, so a pair at +inf keeps its two clusters apart for good and more may be left.
 * merge_a[t] < merge_b[t], merge_distance[t] and merge_size[t], n - 1 entries each, receive the merges in the order performed.  The heights are non-decreasing exactly for single and complete; for average they
 * are non-decreasing up to the rounding of the update, and nothing more is promised.  merge_a / merge_b are members of the two
 * clusters (their smallest): a union-find over the merges in order rebuilds every cluster.  Under HULK_LINKAGE_SINGLE the heights are
 * hulk_dendrogram's edge distances as a multiset and every cut gives hulk_cluster's labels; hulk_dendrogram computes that tree without
 * the matrix.  A function of the inputs alone, however many distances tie: launch shapes, chunks and scheduling cannot change a bit.
 * The n x n matrix lives on the device only: 8 * n * n bytes (n at most HULK_LINKAGE_MAX_N) beside the set; free device memory is
 * checked before anything is allocated, and a matrix that does not fit is refused with HULK_ERR_HIP and a text that names the bytes
 * needed.  hulk_smash's matrix kernel fills D, k_linkage_sym (hulk_linkage.hip) makes W in place; per row the nearest live neighbour
 * behind it is cached under the key, and every merge is three launches of fixed shape (k_linkage_pick, k_linkage_update,
 * k_linkage_rescan) that take p, q and "finished" from device memory: the host queues them without a synchronisation per merge and
 * looks at "finished" once per 4096 merges.
 * HULK_ERR_ARG before any HIP call, with a text in hulk_last_error(NULL): NULL arrays (weights may be NULL for bottomk), opts or
 * n_merges; n or sketch_size == 0; an unknown metric or method; bottomk above HULK_MINHASH_MAX_SKETCH; non-zero flags or reserved; n
 * above HULK_LINKAGE_MAX_N.  n == 1 is valid: 0 merges. */
#define HULK_LINKAGE_SINGLE 0
#define HULK_LINKAGE_COMPLETE 1
#define HULK_LINKAGE_AVERAGE 2
#define HULK_LINKAGE_MAX_N 65536u
typedef struct hulk_linkage_opts {
    int metric;            /* HULK_METRIC_JACCARD / HULK_METRIC_WEIGHTED_JACCARD / HULK_METRIC_BOTTOMK */
    int method;            /* HULK_LINKAGE_SINGLE / HULK_LINKAGE_COMPLETE / HULK_LINKAGE_AVERAGE */
    uint32_t flags;        /* zero */
    uint64_t reserved[4];  /* zero */
} hulk_linkage_opts;
typedef struct hulk_linkage_stats {
    double seconds_total, kernel_ms_matrix, kernel_ms_merge;   /* the whole call; the matrix kernel and k_linkage_sym; the cache's first fill and every merge (HIP events around each phase) */
    uint32_t merges, components;
    uint64_t rows_rescanned;   /* rows k_linkage_rescan scanned, the n of the first fill included */
} hulk_linkage_stats;
int hulk_linkage(int device, const uint64_t *mins, const double *weights, uint32_t n, uint32_t sketch_size,
                 const hulk_linkage_opts *opts, uint32_t *merge_a, uint32_t *merge_b, double *merge_distance,
                 uint32_t *merge_size /* n - 1 each */, uint32_t *n_merges, hulk_linkage_stats *stats);
/* The directory form: hulk_dendrogram_files' loader, error texts and their order, metric and algo names and checks; method:
 * "single" | "complete" | "average".  merge_a / merge_b / merge_distance / merge_size [unique paths - 1] and n_merges may be NULL.
 * csv_path != NULL: hulk_dendrogram_files' file — the header "merge,sketch_a,sketch_b,distance,similarity,size" and one line per
 * merge in the order performed.  cut_distance in [0, 1] and cut_csv_path != NULL: "sketch,cluster,size,representative" for the
 * clusters that the merges with distance <= cut_distance build (a union-find over them, labels the smallest members); cut_distance
 * NaN: no cut; any other cut_distance, or one in [0, 1] without a cut_csv_path, is HULK_ERR_ARG. */
int hulk_linkage_files(int device, const char *const *paths, uint32_t n, uint32_t ksize, const char *algo, const char *metric,
                       const char *method, uint32_t threads, const char *csv_path, double cut_distance /* NaN: no cut */,
                       const char *cut_csv_path, uint32_t *merge_a, uint32_t *merge_b, double *merge_distance, uint32_t *merge_size,
                       uint32_t *n_merges, hulk_linkage_stats *stats, char *errbuf, uint64_t errbuf_len);

/* ---- a banded index over a sketch collection: hulk_search at a distance threshold against a database that stays on the device ------
 * The distance is hulk_smash's jaccard and nothing else: mins compared as (double)min, distance = 1.0 - (double)equal / (double)S.
 * weightedjaccard and bottomk are HULK_ERR_ARG with a text: a weighted distance (or a set similarity) does not bound the number of
 * unequal slots, so the filter below would not be exact for them.
 * BANDS.  For the build threshold D = opts->max_distance in [0, 1), u_max is the largest u in [0, S] with
 * 1.0 - (double)(S - u) / (double)S <= D — the distance expression itself in fp64, so the bound and the kernel cannot disagree about
 * an edge case.  bands = 0 derives B = u_max + 1; band b covers the slots [floor(b S / B), floor((b + 1) S / B)).  u_max == S (D = 1)
 * is HULK_ERR_ARG, "every sketch is within this distance: use hulk_search".  bands may be given, 1 .. S; below u_max + 1 the index is
 * an ordinary LSH filter, faster and incomplete: the result is what RESULT says and nothing more.
 * KEYS.  key(sketch, b) folds the band's slots in ascending order: h = 0, then h = hash64(h ^ bits((double)min[t]), ~0) with the
 * minimap2 mix this library hashes k-mers with.  The hash is over the double's bits: two mins that smash calls equal get one key.
 * CANDIDATES.  Database sketch p is a candidate of query q when key(q, b) == key(p, b) for at least one b.  A 64-bit collision makes
 * a candidate that a slot-by-slot compare would not; its real distance is computed anyway, so a collision adds work and never changes
 * a result.
 * RESULT.  For every query hulk_search's hit list (k <= HULK_SEARCH_MAX_K, ordered by (distance, database index), the entries behind
 * hit_count 0xFFFFFFFF / NaN) computed over the candidates only, with the limit max_distance of the search (negative or NaN: the
 * build's D; above the build's D: HULK_ERR_ARG, whatever bands is).  HULK_SEARCH_SELF: q_mins NULL, m ignored, the queries are the
 * indexed set and (i, i) is left out.  Every distinct candidate pair is verified and counted once, however many bands it shares:
 * stats->candidates is the number of distinct (q, p) pairs, stats->within how many of them were within the limit before the cut to
 * k — a caller can see a truncated list.
 * THEOREM.  With bands >= u_max + 1 (the default) the result is hulk_search(metric jaccard, the same k, the same max_distance) over
 * the whole database, bit for bit.  (Two sketches within D differ in at most u_max slots; these lie in at most u_max of the
 * u_max + 1 disjoint bands, so one band is intact and its keys are equal: every pair within the limit is a candidate, and a
 * candidate's distance is the bits of hulk_search's.)
 * The index keeps on the device the mins as doubles [n][S], the keys by sketch [n][B] and per band the (key, sketch) pairs sorted by
 * (key, sketch): 8 S + 20 B bytes a sketch (hulk_index_info's device_bytes); a build that does not fit is HULK_ERR_HIP with the
 * bytes needed.  A search launches k_index_keys (the queries' keys), k_index_probe twice around k_index_scan (per (query, band) a
 * binary search for the run of equal keys; count, one synchronisation in which the host reads the candidates per query, then every
 * candidate to its final slot — no atomics, no sort), k_index_verify and k_index_select (hulk_index.hip).  scratch_bytes (0 = 256 MiB)
 * holds the candidates, 16 bytes each: the queries are cut into blocks that fit it, a single query above it goes in pieces; neither
 * can change a byte of the result.  The buffers of a search stay allocated between calls (beside device_bytes).
 * On the HOST the handle keeps a copy of the raw mins, 8 * n * sketch_size bytes (what hulk_index_save writes), and the names, for its
 * whole life; a build, load or search that cannot allocate host memory is HULK_ERR_HIP with "out of host memory", not an abort.
 * LIMITS.  A launch stays below HIP's 2^32 threads whatever the shape: a wave serves a (query, band) of the probe and a candidate of the
 * verification, so the count pass runs over chunks of 2^25 / bands queries, a block holds at most that many queries and at most 2^25
 * candidates (a scratch_bytes above 512 MiB changes nothing), and what is left is refused with HULK_ERR_ARG before any HIP call:
 * n * bands and m * bands (the keys: a thread per sketch and band) must be below 2^32, bands at most 65535 (hulk_index_plan.h).
 * Every call returns synchronised (the outputs are host arrays) and works on the null stream of the index's device.  One call at a
 * time per index; hulk_index_free ends its life (NULL is fine).
 * HULK_ERR_ARG before any HIP call, with a text in hulk_last_error(NULL): NULL pointers; n, m or sketch_size == 0; a metric other than
 * HULK_METRIC_JACCARD; max_distance outside [0, 1) at a build; bands above sketch_size (or 65535); k == 0 or above HULK_SEARCH_MAX_K;
 * unknown flags; non-zero reserved; queries together with HULK_SEARCH_SELF or neither; a scratch_bytes below one candidate; the two
 * products of LIMITS.  The text of a max_distance above the build's prints both doubles as %.17g: -j 0.90 builds for
 * 0.099999999999999978, which a later --maxDistance 0.1 is above. */
typedef struct hulk_index hulk_index;
typedef struct hulk_index_opts {
    double max_distance;     /* D in [0, 1): the largest distance a search may ask for */
    uint32_t bands;          /* 0 = u_max + 1 (exact); 1 .. sketch_size */
    int metric;              /* HULK_METRIC_JACCARD (0) */
    uint32_t flags;          /* zero */
    uint32_t pad;            /* zero */
    uint64_t reserved[4];    /* zero */
} hulk_index_opts;
typedef struct hulk_index_search_opts {
    uint32_t k;              /* hits per query, 1 .. HULK_SEARCH_MAX_K */
    uint32_t flags;          /* HULK_SEARCH_SELF */
    double max_distance;     /* in [0, D]; negative or NaN: D */
    uint64_t scratch_bytes;  /* 0 = default */
    uint64_t reserved[4];    /* zero */
} hulk_index_search_opts;
typedef struct hulk_index_search_stats {
    double seconds_total;    /* the whole call */
    double kernel_ms_keys;   /* the queries' upload and k_index_keys (HIP events, as the three below) */
    double kernel_ms_probe;  /* k_index_probe (count and fill) and k_index_scan */
    double kernel_ms_verify; /* k_index_verify */
    double kernel_ms_select; /* k_index_select */
    uint64_t candidates;     /* distinct (query, sketch) pairs that share a band */
    uint64_t within;         /* ... of which within the limit, before the cut to k */
    uint32_t query_blocks, pieces;   /* pieces: the parts of queries whose candidates exceed the scratch (0: none did) */
} hulk_index_search_stats;
int hulk_index_build(int device, const uint64_t *mins, uint32_t n, uint32_t sketch_size, const hulk_index_opts *opts, hulk_index **index);
int hulk_index_search(hulk_index *index, const uint64_t *q_mins, uint32_t m, const hulk_index_search_opts *opts, uint32_t *hit_index,
                      double *hit_distance, uint32_t *hit_count, hulk_index_search_stats *stats);
int hulk_index_info(const hulk_index *index, uint32_t *n, uint32_t *sketch_size, uint32_t *bands, double *max_distance,
                    uint64_t *device_bytes);   /* HULK_ERR_ARG for NULL; any output may be NULL */
void hulk_index_free(hulk_index *index);
/* The names of the sketches: empty after hulk_index_build until hulk_index_set_names (n must be the index's), the sorted unique paths
 * after hulk_index_build_files, what the file held after hulk_index_load.  hulk_index_name: NULL for NULL or i >= n. */
int hulk_index_set_names(hulk_index *index, const char *const *names, uint32_t n);
const char *hulk_index_name(const hulk_index *index, uint32_t i);
/* One binary file, little-endian: the magic "HULKIDX\n", the format version (1), sketch_size, n, bands (uint32 each), the bits of the
 * threshold, the bytes of the names and of the mins (uint64 each), the names (NUL-terminated), the raw mins [n][sketch_size] and a
 * CRC-32 over all of it.  Loading checks the lengths against the file's and the checksum, then uploads and rebuilds keys and order
 * on the device — the code path of a build — so a loaded index answers every search with the bytes of the one that was saved.  A
 * truncated, corrupt or foreign file is HULK_ERR_IO with a text, before any HIP call: never a crash, never a partly loaded index. */
int hulk_index_save(const hulk_index *index, const char *path);
int hulk_index_load(int device, const char *path, hulk_index **index);
/* The file forms.  hulk_index_build_files: the files go through hulk_load_sketches' loader (MD5, FindSketch, the reference's error
 * texts; a set of ONE sketch is valid); the sorted unique paths become the names.  hulk_index_search_files: the query files through
 * the same loader ("sketch length mismatch: %d vs %d\n": the queries', the index's); HULK_SEARCH_SELF in flags: query_paths NULL.
 * csv_path != NULL: hulk_search_files' file, "query,rank,hit,similarity" with the same strings, the hits named by hulk_index_name.
 * hit_index / hit_distance [unique query paths][k] and hit_count may be NULL. */
int hulk_index_build_files(int device, const char *const *paths, uint32_t n, uint32_t ksize, const char *algo, uint32_t threads,
                           const hulk_index_opts *opts, hulk_index **index, char *errbuf, uint64_t errbuf_len);
int hulk_index_search_files(hulk_index *index, const char *const *query_paths, uint32_t n_q, uint32_t ksize, const char *algo,
                            uint32_t threads, const hulk_index_search_opts *opts, const char *csv_path, uint32_t *hit_index,
                            double *hit_distance, uint32_t *hit_count, hulk_index_search_stats *stats, char *errbuf, uint64_t errbuf_len);

/* Device self-test: the jump hash replaces the fp64 division 2^31/r by a Newton reciprocal; this
 * checks RN(1/r) against IEEE division for EVERY r in [1, 2^31] and returns the mismatch count. */
int hulk_selftest_reciprocal(hulk_ctx *ctx, uint64_t *mismatches);

/* Exact pruning of the CWS table scan (no concept drift): a 256-bin x 8-slot tile of K is only read when
 * min(K) * max(1/f) (or min(K) * min(1/f) for min(K) >= 0) can get below one of its slots' current weights —
 * AddElement only replaces a weight by a smaller A (histosketch.go:139-153), so the sketch is unchanged.
 * Reports how many tiles the scans read out of how many they covered (both cumulative). */
int hulk_get_scan_stats(hulk_ctx *ctx, uint64_t *tiles_visited, uint64_t *tiles_total);

/* Per-kernel timing for bench.py: when enabled, hipEvents bracket every launch of the heavy kernels
 * ("k_minimizer_fast", "k_jump_bin", "k_cws_scan", "k_cmsd_freq"; each alone) on the stream they are launched on.
 * enabled: 0 off, 1 all of them, otherwise a mask (2 k_minimizer_fast, 4 k_jump_bin, 8 k_cws_scan, 16 k_cmsd_freq,
 * 32 every launch: hulk_get_profile_table)
 * "k_jump_left" stays a valid name for hulk_get_profile (ABI 4): that kernel is gone, its chains are finished inside k_jump_bin,
 * so it reports zero launches and 0 ms.
 * — every bracketed launch costs the stream two event records (~3 % of a C2 step for all of them), so the timed pass of
 * bench.py brackets nothing and the durations come from a separate pass. */
int hulk_set_profiling(hulk_ctx *ctx, int enabled);
/* Number of timed launches of `kernel` and their summed duration (synchronises; clears that log). */
int hulk_get_profile(hulk_ctx *ctx, const char *kernel, uint64_t *launches, double *total_ms);
/* hulk_set_profiling bit 32: EVERY kernel launch of the step path (binning chain and flush) is timed — an event in front of each
 * launch, a kernel's duration = the time to the next event on its stream — meant for HULK_FLAG_NO_OVERLAP contexts, where every
 * kernel runs alone.  Writes "kernel<TAB>launches<TAB>total_ms<LF>" lines (NUL-terminated) into `out` (HULK_ERR_ARG if `cap`
 * is too small), synchronises, clears the log. */
int hulk_get_profile_table(hulk_ctx *ctx, char *out, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* HULK_HIP_H */
