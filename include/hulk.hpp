// hulk.hpp — C++ host side above the C ABI (hulk_hip.h): the reference's Go objects for the sketch
// path, with the reference's method names, argument meaning and error texts.
//
//   reference (Go)                                                        here
//   -------------------------------------------------------------------   ---------------------------
//   pipeline.Info / SketchCmd          src/pipeline/pipeline.go           hulk::SketchInfo
//   findMinimizers(chan, *Info)        src/pipeline/boss.go:54            hulk::Boss::FindMinimizers
//   theBoss.AddSeq / Flush / StopWork / GetMinimizerCount   boss.go:24-41 same names on hulk::Boss
//   histosketch.HistoSketch (exported fields)  histosketch.go:36-47       hulk::HistoSketch
//   DataStreamer + FastqHandler + AddSeq loop  pipeline/sketch.go:40-217  hulk::Boss::SketchFiles
//   log.Fatalf("ERROR---> %v") via helpers.ErrorCheck   helpers.go:31-35  hulk::Error (what() = %v)
//   SeqMinimizer.Run's loop with the read stream sharded over GPUs        hulk::Boss::Shard + AddSeq + StopWorkSharded
//       pipeline/sketch.go:182-250                                          (RCCL inside libhulkhip.so)
//   `--stream`: "prints the sketches ... after every interval"            hulk::Boss::EnableSnapshots / CollectSnapshots /
//       cmd/sketch.go:56 (promised, read nowhere in src/pipeline)           OnSnapshot (recorded inside the batched flush)
//   (none: the k nearest sketches of a database for every query sketch)   hulk::Search (HULKdata.GetDistance per pair)
//   (none: the same hits within a distance from a banded index on the GPU)  hulk::Index (Build / BuildFiles / Load / Save / Search / SearchSelf)
//   (none: the sketches of a collection grouped at a distance threshold)  hulk::Cluster / hulk::ClusterFiles (single linkage)
//   (none: every threshold at once, the single-linkage dendrogram)         hulk::Dendrogram / hulk::DendrogramFiles
//   (none: the complete- and average-linkage dendrograms the paper's       hulk::Linkage / hulk::LinkageFiles
//       notebooks draw with sns.clustermap from `smash`'s matrix)
//
// Header only; link with -lhulkhip.  A Boss is single-caller, like SeqMinimizer.Run's goroutine.
#ifndef HULK_HPP
#define HULK_HPP

#include <algorithm>
#include <array>
#include <cstdint>
#include <exception>
#include <functional>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "hulk_hip.h"

namespace hulk {

class Error : public std::runtime_error {
 public:
    Error(int code, const std::string &msg) : std::runtime_error(msg), code_(code) {}
    int code() const { return code_; }
 private:
    int code_;
};

// the flags of `hulk sketch` that reach the path (cmd/sketch.go:50-59, cmd/root.go:62)
struct SketchInfo {
    unsigned KmerSize = 21;        // -k
    unsigned WindowSize = 9;       // -w
    unsigned SketchSize = 50;      // -s
    unsigned Interval = 0;         // -i
    double DecayRatio = 1.0;       // -x
    int32_t SpectrumSize = 0;      // 0 = Pow(KmerSize, 4)  (cmd/sketch.go:118)
    int Device = 0;
    bool KMV = false, KHF = false; // feed the MinHash sketches (HULK_FLAG_KMV / HULK_FLAG_KHF): the reference's boss constructs
                                   // both and never feeds them (boss.go:18-19); Boss::CollectKMVsketch / CollectKHFsketch need these
    unsigned Rank = 0, World = 1;  // multi-GPU: this process is rank Rank of World (one GPU each); it owns the sketch
                                   // slots [S*Rank/World, S*(Rank+1)/World) and Boss::Shard connects it to the others
};
using UniqueId = std::array<uint8_t, HULK_UNIQUE_ID_BYTES>;

// histosketch.HistoSketch as sketchio consumes it (exported fields only)
struct HistoSketch {
    unsigned KmerSize = 0;
    std::vector<uint64_t> Sketch;          // `mins`
    std::vector<double> SketchWeights;     // `weights`
    unsigned SketchSize = 0;               // `num`
    int32_t Dimensions = 0;                // `num_histogram_bins`
    bool ApplyConceptDrift = false;        // `concept_drift` (decayRatio != 1.0, histosketch.go:79-81)
};

// the histosketch as it stood after flushed spectrum `Ordinal` (1-based), `Reads` reads into the stream
struct Snapshot {
    uint64_t Ordinal = 0, Reads = 0; HistoSketch Sketch;
    std::vector<double> Distances;      // to the sketches of Boss::SetPanel, in the panel's order; empty without a panel
};

struct IngestStats { uint64_t SeqCount = 0, LengthTotal = 0, Lines = 0, BytesIn = 0; double Seconds = 0; };

class Boss {
 public:
    // findMinimizers + NewHistoSketch: throws hulk::Error with the reference's message
    static Boss FindMinimizers(const SketchInfo &info) { return Boss(info); }

    Boss(Boss &&o) noexcept : ctx_(o.ctx_), info_(o.info_), bins_(o.bins_), sharded_(o.sharded_), panel_(o.panel_), bases_(std::move(o.bases_)),
                              offsets_(std::move(o.offsets_)), snap_(std::move(o.snap_)) { o.ctx_ = nullptr; o.panel_ = 0; }
    Boss(const Boss &) = delete;
    Boss &operator=(const Boss &) = delete;
    ~Boss() { if (ctx_) hulk_destroy(ctx_); }

    // ---- the read stream sharded over World GPUs (include/hulk_hip.h, hulk_step_sharded): rank 0 draws an id
    // (CommUniqueId), the host hands it to the other ranks, every rank calls Shard — then AddSeq takes THIS RANK's reads:
    // of every step of World * T sketching intervals of the global stream (T = hulk_batch_size) the whole intervals
    // [Rank * T, (Rank + 1) * T), in stream order.  A full share (T * Interval reads) is pushed as one step.
    static UniqueId CommUniqueId() {
        UniqueId id{};
        const int rc = hulk_comm_unique_id(id.data());
        if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
        return id;
    }
    void Shard(const UniqueId &id) {
        if (info_.Interval == 0) throw Error(HULK_ERR_ARG, "a sharded run needs Interval > 0");
        check(hulk_comm_init(ctx_, id.data(), info_.Rank, info_.World));
        sharded_ = true;
    }
    // End of the stream: `lastStepIntervals` = sketching intervals of the GLOBAL stream in the last, ragged step (the same
    // value on every rank, 0 if the stream ended on a step border); this rank's remaining reads are its share of it.
    void StopWorkSharded(uint32_t lastStepIntervals) {
        if (lastStepIntervals) push_step(lastStepIntervals);
        check(hulk_finish(ctx_));
    }

    // theBoss.AddSeq (boss.go:24-26); sequences are staged and cross the ABI in batches
    void AddSeq(const uint8_t *seq, size_t len) {
        bases_.insert(bases_.end(), seq, seq + len);
        offsets_.push_back(bases_.size());
        if (sharded_) {
            if (offsets_.size() - 1 == (size_t)hulk_batch_size(ctx_) * info_.Interval) push_step(info_.World * hulk_batch_size(ctx_));
        } else if (offsets_.size() > kBatchReads || bases_.size() > kBatchBytes) push();
    }
    void AddSeq(const std::string &seq) { AddSeq(reinterpret_cast<const uint8_t *>(seq.data()), seq.size()); }

    // theBoss.Flush (boss.go:34-36).  With Interval set the library applies the rule of sketch.go:211-215
    // itself; an explicit Flush is only meaningful when Interval == 0.
    void Flush() { push(); check(hulk_flush(ctx_)); }

    // final Flush + theBoss.StopWork (sketch.go:219-224)
    void StopWork() { push(); check(hulk_finish(ctx_)); }

    // theBoss.GetMinimizerCount (boss.go:39-41)
    uint64_t GetMinimizerCount() {
        uint64_t r = 0, m = 0, l = 0;
        check(hulk_get_counters(ctx_, &r, &m, &l));
        return m;
    }

    // DataStreamer.Run + FastqHandler.Run + the AddSeq loop, natively (paths empty = STDIN)
    IngestStats SketchFiles(const std::vector<std::string> &paths, bool fasta = false, unsigned threads = 0) {
        push();
        std::vector<const char *> p;
        for (const auto &s : paths) p.push_back(s.c_str());
        hulk_ingest_stats st{};
        check(hulk_sketch_files(ctx_, p.empty() ? nullptr : p.data(), (uint32_t)p.size(), fasta ? 1 : 0, threads, &st));
        IngestStats out;
        out.SeqCount = st.n_seqs; out.LengthTotal = st.total_len; out.Lines = st.n_lines; out.BytesIn = st.bytes_in;
        out.Seconds = st.seconds;
        return out;
    }

    // the Sketcher's HistoSketch (sketch.go:271-301), valid after StopWork
    HistoSketch Sketch() {
        HistoSketch hs;
        hs.KmerSize = info_.KmerSize; hs.SketchSize = info_.SketchSize; hs.Dimensions = bins_;
        hs.ApplyConceptDrift = info_.DecayRatio != 1.0;
        hs.Sketch.resize(info_.SketchSize); hs.SketchWeights.resize(info_.SketchSize);
        check(sharded_ ? hulk_gather_sketch(ctx_, hs.Sketch.data(), hs.SketchWeights.data())
                       : hulk_get_sketch(ctx_, hs.Sketch.data(), hs.SketchWeights.data()));
        return hs;
    }

    // theBoss.CollectKMVsketch / CollectKHFsketch (boss.go:44-51) of a Boss created with SketchInfo.KMV / .KHF: the signature
    // over every read added so far — KMV: the SketchSize smallest values of the multiset, ascending (fewer while fewer were
    // fed); KHF: SketchSize slots.  Without the flag: hulk::Error(HULK_ERR_STATE).
    std::vector<uint64_t> CollectKMVsketch() { return collect(HULK_MINHASH_KMV); }
    std::vector<uint64_t> CollectKHFsketch() { return collect(HULK_MINHASH_KHF); }
    // MinHash.Merge (khf.go:49-55): fold another Boss's signature (another rank's share of the stream) into this one's
    void MergeKMVsketch(const std::vector<uint64_t> &mins) { push(); check(hulk_minhash_merge(ctx_, HULK_MINHASH_KMV, mins.data(), (uint32_t)mins.size())); }
    void MergeKHFsketch(const std::vector<uint64_t> &mins) { push(); check(hulk_minhash_merge(ctx_, HULK_MINHASH_KHF, mins.data(), (uint32_t)mins.size())); }

    // ---- sketch snapshots (hulk_set_snapshots): the sketch after every `every`-th flushed spectrum, recorded on the GPU inside
    // the batched flush — what batch = 1 and Sketch() after every interval would give, without giving up the batch.  Call before
    // the first AddSeq; capacity = snapshots the device ring holds (0 = the library's default).  Not with Shard().
    void EnableSnapshots(uint32_t every, uint32_t capacity = 0) {
        check(hulk_set_snapshots(ctx_, every, capacity));
        panel_ = 0;                        // (setting the snapshots again drops a panel: hulk_set_panel)
    }
    // every snapshot the ring still holds, in stream order (synchronises, like Sketch())
    std::vector<Snapshot> CollectSnapshots() {
        push();
        uint64_t recorded = 0, first = 0;
        check(hulk_snapshot_count(ctx_, &recorded, &first));
        const uint32_t n = (uint32_t)(recorded - first), S = info_.SketchSize;
        std::vector<hulk_snapshot_info> inf(n ? n : 1);
        std::vector<uint64_t> mins((size_t)n * S + 1);
        std::vector<double> weights((size_t)n * S + 1);
        check(hulk_get_snapshots(ctx_, first, n, inf.data(), mins.data(), weights.data()));
        std::vector<double> dist((size_t)n * panel_ + 1);
        if (panel_) check(hulk_get_snapshot_distances(ctx_, first, n, dist.data()));
        std::vector<Snapshot> out(n);
        for (uint32_t i = 0; i < n; i++) {
            fill(out[i], inf[i], mins.data() + (size_t)i * S, weights.data() + (size_t)i * S);
            out[i].Distances.assign(dist.data() + (size_t)i * panel_, dist.data() + (size_t)(i + 1) * panel_);
        }
        return out;
    }
    // ---- a panel of reference sketches (hulk_set_panel): every snapshot is scored against it on the GPU, where it is recorded,
    // and carries the result in Snapshot::Distances — HULKdata.GetDistance as Smash() computes it.  metric: "jaccard" |
    // "weightedjaccard"; snapshotIsSubject: the snapshot's row of the matrix smash would print (its weights), else its column
    // (the panel's weights).  After EnableSnapshots, before the first AddSeq; an empty panel removes it.
    void SetPanel(const std::vector<HistoSketch> &panel, const std::string &metric = "jaccard", bool snapshotIsSubject = true) {
        if (metric != "jaccard" && metric != "weightedjaccard") throw Error(HULK_ERR_ARG, "supplied distance metric is not available: " + metric);
        const uint32_t N = (uint32_t)panel.size(), S = N ? panel[0].SketchSize : info_.SketchSize;
        std::vector<uint64_t> mins((size_t)N * S + 1);
        std::vector<double> weights((size_t)N * S + 1);
        for (uint32_t i = 0; i < N; i++) {
            if (panel[i].Sketch.size() != S || panel[i].SketchWeights.size() != S) throw Error(HULK_ERR_ARG, "sketch length mismatch");
            std::copy(panel[i].Sketch.begin(), panel[i].Sketch.end(), mins.begin() + (size_t)i * S);
            std::copy(panel[i].SketchWeights.begin(), panel[i].SketchWeights.end(), weights.begin() + (size_t)i * S);
        }
        check(hulk_set_panel(ctx_, mins.data(), weights.data(), N, S, metric == "weightedjaccard" ? HULK_METRIC_WEIGHTED_JACCARD : HULK_METRIC_JACCARD,
                             snapshotIsSubject ? HULK_PANEL_ROW : HULK_PANEL_COLUMN));
        panel_ = N;
    }
    // fn gets every snapshot once, in stream order, on the caller's thread, from inside AddSeq / Flush / SketchFiles / PollSnapshots /
    // StopWork as soon as the flush that recorded it is found complete (nothing on the step path waits for it).  An exception thrown
    // by fn ends the run: it is rethrown from the call that delivered the snapshot.  After EnableSnapshots, before the first AddSeq.
    void OnSnapshot(std::function<void(const Snapshot &)> fn) {
        auto st = std::make_unique<SnapState>();
        st->fn = std::move(fn); st->owner_info = info_; st->bins = bins_;
        check(hulk_set_snapshot_panel_callback(ctx_, &Boss::snap_thunk, st.get()));     // (Distances stay empty without a panel)
        snap_ = std::move(st);
    }
    // hands the snapshots of every flush that has run to the OnSnapshot function; never blocks; returns how many
    uint32_t PollSnapshots() { uint32_t n = 0; check(hulk_poll_snapshots(ctx_, &n)); return n; }

    hulk_ctx *handle() { return ctx_; }

 private:
    static constexpr size_t kBatchReads = 1u << 16, kBatchBytes = 64u << 20;
    explicit Boss(const SketchInfo &info) : info_(info) {
        hulk_params p{};
        p.k = info.KmerSize; p.w = info.WindowSize; p.sketch_size = info.SketchSize; p.num_bins = info.SpectrumSize;
        p.decay_ratio = info.DecayRatio; p.interval = info.Interval; p.device = info.Device;
        p.flags = (info.KMV ? HULK_FLAG_KMV : 0u) | (info.KHF ? HULK_FLAG_KHF : 0u);
        if (info.World > 1) {
            p.slot_begin = (uint32_t)((uint64_t)info.SketchSize * info.Rank / info.World);
            p.slot_count = (uint32_t)((uint64_t)info.SketchSize * (info.Rank + 1) / info.World) - p.slot_begin;
        }
        const int rc = hulk_create(&p, &ctx_);
        if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
        bins_ = info.SpectrumSize;
        if (bins_ == 0) { uint64_t b = 1; for (int i = 0; i < 4; i++) b *= info.KmerSize; bins_ = (int32_t)b; }
        offsets_.push_back(0);
    }
    void push() {
        const uint64_t n = offsets_.size() - 1;
        if (n == 0) return;
        const int rc = hulk_add_reads(ctx_, bases_.data(), offsets_.data(), n);
        bases_.clear(); offsets_.assign(1, 0);
        check(rc);
    }
    void push_step(uint32_t stepIntervals) {
        const uint64_t n = offsets_.size() - 1;
        const int rc = hulk_step_sharded_host(ctx_, bases_.data(), offsets_.data(), n, stepIntervals);
        bases_.clear(); offsets_.assign(1, 0);
        check(rc);
    }
    void check(int rc) {
        if (snap_ && snap_->thrown) { std::exception_ptr e = snap_->thrown; snap_->thrown = nullptr; std::rethrow_exception(e); }
        if (rc != HULK_OK) throw Error(rc, hulk_last_error(ctx_));
    }
    struct SnapState { std::function<void(const Snapshot &)> fn; SketchInfo owner_info; int32_t bins = 0; std::exception_ptr thrown; };
    static void fill(Snapshot &s, const SketchInfo &info, int32_t bins, const hulk_snapshot_info &inf, const uint64_t *mins, const double *weights) {
        s.Ordinal = inf.ordinal; s.Reads = inf.n_reads;
        s.Sketch.KmerSize = info.KmerSize; s.Sketch.SketchSize = info.SketchSize; s.Sketch.Dimensions = bins;
        s.Sketch.ApplyConceptDrift = info.DecayRatio != 1.0;
        s.Sketch.Sketch.assign(mins, mins + info.SketchSize); s.Sketch.SketchWeights.assign(weights, weights + info.SketchSize);
    }
    void fill(Snapshot &s, const hulk_snapshot_info &inf, const uint64_t *mins, const double *weights) { fill(s, info_, bins_, inf, mins, weights); }
    static int snap_thunk(void *user, const hulk_snapshot_info *inf, const uint64_t *mins, const double *weights, uint32_t,
                          const double *distances, uint32_t n_panel) {
        SnapState *st = static_cast<SnapState *>(user);
        try {
            Snapshot s; fill(s, st->owner_info, st->bins, *inf, mins, weights);
            if (n_panel) s.Distances.assign(distances, distances + n_panel);
            st->fn(s); return 0;
        }
        catch (...) { st->thrown = std::current_exception(); return 1; }             // (no exception crosses the C ABI)
    }
    std::vector<uint64_t> collect(int algo) {
        push();
        std::vector<uint64_t> mins(info_.SketchSize ? info_.SketchSize : 1);
        uint32_t n = 0;
        check(hulk_get_minhash(ctx_, algo, mins.data(), &n, nullptr));
        mins.resize(n);
        return mins;
    }

    hulk_ctx *ctx_ = nullptr;
    SketchInfo info_;
    int32_t bins_ = 0;
    bool sharded_ = false;
    uint32_t panel_ = 0;                   // SetPanel: sketches in the panel
    std::vector<uint8_t> bases_;
    std::vector<uint64_t> offsets_;
    std::unique_ptr<SnapState> snap_;      // OnSnapshot: lives on the heap, the library holds its address
};

// the metric names of Smash, Search, Cluster and Dendrogram -> HULK_METRIC_*.  "bottomk" is the estimator of KMV sketches
// (KMVsketch.GetSimilarity, the multiset intersection of the two value lists as uint64; HistoSketch::Sketch carries the values,
// SketchWeights is not read); the *Files forms take it with algo "kmv" only
inline int MetricCode(const std::string &metric) {
    if (metric == "jaccard") return HULK_METRIC_JACCARD;
    if (metric == "weightedjaccard") return HULK_METRIC_WEIGHTED_JACCARD;
    if (metric == "bottomk") return HULK_METRIC_BOTTOMK;
    throw Error(HULK_ERR_ARG, "supplied distance metric is not available: " + metric);
}

namespace detail {
// the Sketch and SketchWeights of a collection as [N][S] arrays (one element more: never empty), S = the first sketch's SketchSize
inline void Pack(const std::vector<HistoSketch> &sketches, std::vector<uint64_t> &mins, std::vector<double> &weights) {
    const uint32_t N = (uint32_t)sketches.size(), S = N ? sketches[0].SketchSize : 0;
    mins.assign((size_t)N * S + 1, 0);
    weights.assign((size_t)N * S + 1, 0.0);
    for (uint32_t i = 0; i < N; i++) {
        if (sketches[i].Sketch.size() != S || sketches[i].SketchWeights.size() != S)
            throw Error(HULK_ERR_ARG, "sketch length mismatch: " + std::to_string(S) + " vs " + std::to_string(sketches[i].Sketch.size()) + "\n");
        std::copy(sketches[i].Sketch.begin(), sketches[i].Sketch.end(), mins.begin() + i * (size_t)S);
        std::copy(sketches[i].SketchWeights.begin(), sketches[i].SketchWeights.end(), weights.begin() + i * (size_t)S);
    }
}
// the C strings of the *_files entry points' paths
inline std::vector<const char *> CPaths(const std::vector<std::string> &files) {
    std::vector<const char *> ptr;
    for (const auto &f : files) ptr.push_back(f.c_str());
    return ptr;
}
// the order the library's loader gives the files (a path given twice counts once)
inline std::vector<std::string> SortedUnique(std::vector<std::string> files) {
    std::sort(files.begin(), files.end());
    files.erase(std::unique(files.begin(), files.end()), files.end());
    return files;
}
}  // namespace detail

// sketchio's pairwise distances over loaded sketches (cmd/smash.go:183-226): distances[s*N+q]
inline std::vector<double> Smash(const std::vector<HistoSketch> &sketches, const std::string &metric, int device = 0) {
    const uint32_t N = (uint32_t)sketches.size(), S = N ? sketches[0].SketchSize : 0;
    std::vector<uint64_t> mins((size_t)N * S);
    std::vector<double> weights((size_t)N * S), out((size_t)N * N);
    for (uint32_t i = 0; i < N; i++) {
        if (sketches[i].Sketch.size() != S) throw Error(HULK_ERR_ARG, "sketch length mismatch");
        for (uint32_t j = 0; j < S; j++) { mins[(size_t)i * S + j] = sketches[i].Sketch[j]; weights[(size_t)i * S + j] = sketches[i].SketchWeights[j]; }
    }
    const int m = MetricCode(metric);
    const int rc = hulk_smash(device, mins.data(), weights.data(), N, S, m, out.data());
    if (rc != HULK_OK) throw Error(rc, hulk_strerror(rc));
    return out;
}

// For every query sketch the k closest sketches of a database, on the GPU (hulk_search): Smash's distance for the pair — queryIsSubject:
// the query's row of that matrix, otherwise the database sketch's column — the pairs that are not NaN (and <= maxDistance, if it is in
// [0, 1]) in (distance, database index) order, at most k per query.  An empty `database` searches the queries among themselves
// (HULK_SEARCH_SELF): a sketch is not its own hit.  The database streams through the device: no queries x database array exists.
struct Hit { uint32_t Index = 0; double Distance = 0; };
inline std::vector<std::vector<Hit>> Search(const std::vector<HistoSketch> &queries, const std::vector<HistoSketch> &database, uint32_t k,
                                            const std::string &metric, bool queryIsSubject = true, double maxDistance = -1.0,
                                            uint64_t scratchBytes = 0, int device = 0, hulk_search_stats *stats = nullptr) {
    const uint32_t M = (uint32_t)queries.size(), P = (uint32_t)database.size(), S = M ? queries[0].SketchSize : 0;
    auto pack = [S](const std::vector<HistoSketch> &set, std::vector<uint64_t> &mins, std::vector<double> &weights, unsigned first) {
        mins.resize(set.size() * (size_t)S); weights.resize(set.size() * (size_t)S);
        for (size_t i = 0; i < set.size(); i++) {
            if (set[i].Sketch.size() != S || set[i].SketchWeights.size() != S)
                throw Error(HULK_ERR_ARG, "sketch length mismatch: " + std::to_string(first) + " vs " + std::to_string(set[i].Sketch.size()) + "\n");
            std::copy(set[i].Sketch.begin(), set[i].Sketch.end(), mins.begin() + i * (size_t)S);
            std::copy(set[i].SketchWeights.begin(), set[i].SketchWeights.end(), weights.begin() + i * (size_t)S);
        }
    };
    std::vector<uint64_t> qm, dm;
    std::vector<double> qw, dw;
    pack(queries, qm, qw, S);
    pack(database, dm, dw, S);
    hulk_search_opts o = hulk_search_opts();
    o.k = k; o.role = queryIsSubject ? HULK_PANEL_ROW : HULK_PANEL_COLUMN; o.flags = P ? 0u : HULK_SEARCH_SELF;
    o.max_distance = maxDistance; o.scratch_bytes = scratchBytes;
    o.metric = MetricCode(metric);
    const size_t kk = k ? k : 1;
    std::vector<uint32_t> index(M * kk + 1), count((size_t)M + 1);
    std::vector<double> distance(M * kk + 1);
    const int rc = hulk_search(device, qm.data(), qw.data(), M, P ? dm.data() : nullptr, P ? dw.data() : nullptr, P, S, &o, index.data(),
                               distance.data(), count.data(), stats);
    if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
    std::vector<std::vector<Hit>> out(M);
    for (uint32_t i = 0; i < M; i++)
        for (uint32_t j = 0; j < count[i]; j++) { Hit h; h.Index = index[i * kk + j]; h.Distance = distance[i * kk + j]; out[i].push_back(h); }
    return out;
}

// A banded index over a collection that stays on the GPU (hulk_index_*): Search's hits under "jaccard" within a distance, computed over
// the sketches that share a band with the query.  Built for maxDistance with bands = 0 (derived) the result is Search(queries, database,
// k, "jaccard", true, limit <= maxDistance), bit for bit; fewer bands make it an LSH filter, faster and incomplete (hulk_hip.h states
// the rule).  The handle is freed with the object; one call at a time per index.
class Index {
public:
    static Index Build(const std::vector<HistoSketch> &sketches, double maxDistance, uint32_t bands = 0, int device = 0) {
        const uint32_t N = (uint32_t)sketches.size(), S = N ? sketches[0].SketchSize : 0;
        hulk_index_opts o = hulk_index_opts();
        o.max_distance = maxDistance; o.bands = bands;
        const std::vector<uint64_t> mins = Pack(sketches, S);
        hulk_index *h = nullptr;
        const int rc = hulk_index_build(device, mins.data(), N, S, &o, &h);
        if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
        return Index(h);
    }
    // the files through the library's loader (MD5, FindSketch, the reference's error texts); the sorted unique paths are the names
    static Index BuildFiles(const std::vector<std::string> &files, double maxDistance, uint32_t bands = 0, uint32_t ksize = 21,
                            const std::string &algo = "histosketch", uint32_t threads = 0, int device = 0) {
        hulk_index_opts o = hulk_index_opts();
        o.max_distance = maxDistance; o.bands = bands;
        const std::vector<const char *> paths = detail::CPaths(files);
        char err[4096] = "";
        hulk_index *h = nullptr;
        const int rc = hulk_index_build_files(device, paths.data(), (uint32_t)paths.size(), ksize, algo.c_str(), threads, &o, &h, err, sizeof err);
        if (rc != HULK_OK) throw Error(rc, err);
        return Index(h);
    }
    static Index Load(const std::string &path, int device = 0) {
        hulk_index *h = nullptr;
        const int rc = hulk_index_load(device, path.c_str(), &h);
        if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
        return Index(h);
    }
    Index(Index &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Index &operator=(Index &&o) noexcept { if (this != &o) { hulk_index_free(h_); h_ = o.h_; o.h_ = nullptr; } return *this; }
    Index(const Index &) = delete;
    Index &operator=(const Index &) = delete;
    ~Index() { hulk_index_free(h_); }

    void Save(const std::string &path) const {
        const int rc = hulk_index_save(h_, path.c_str());
        if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
    }
    // maxDistance < 0: the build's.  (An empty `queries` is the library's "m must be positive", not a self-join: SearchSelf is its own call.)
    std::vector<std::vector<Hit>> Search(const std::vector<HistoSketch> &queries, uint32_t k, double maxDistance = -1.0, uint64_t scratchBytes = 0,
                                         hulk_index_search_stats *stats = nullptr) const {
        const std::vector<uint64_t> mins = Pack(queries, SketchSize());
        return Run(mins.data(), (uint32_t)queries.size(), 0u, k, maxDistance, scratchBytes, stats);
    }
    // the indexed sketches among themselves (HULK_SEARCH_SELF): a sketch is not its own hit
    std::vector<std::vector<Hit>> SearchSelf(uint32_t k, double maxDistance = -1.0, uint64_t scratchBytes = 0,
                                             hulk_index_search_stats *stats = nullptr) const {
        return Run(nullptr, Size(), HULK_SEARCH_SELF, k, maxDistance, scratchBytes, stats);
    }
    uint32_t Size() const { uint32_t v = 0; hulk_index_info(h_, &v, nullptr, nullptr, nullptr, nullptr); return v; }
    uint32_t SketchSize() const { uint32_t v = 0; hulk_index_info(h_, nullptr, &v, nullptr, nullptr, nullptr); return v; }
    uint32_t Bands() const { uint32_t v = 0; hulk_index_info(h_, nullptr, nullptr, &v, nullptr, nullptr); return v; }
    double MaxDistance() const { double v = 0; hulk_index_info(h_, nullptr, nullptr, nullptr, &v, nullptr); return v; }
    uint64_t DeviceBytes() const { uint64_t v = 0; hulk_index_info(h_, nullptr, nullptr, nullptr, nullptr, &v); return v; }
    std::string Name(uint32_t i) const { const char *s = hulk_index_name(h_, i); return s ? s : ""; }
    hulk_index *Handle() const { return h_; }

private:
    explicit Index(hulk_index *h) : h_(h) {}
    std::vector<std::vector<Hit>> Run(const uint64_t *mins, uint32_t M, uint32_t flags, uint32_t k, double maxDistance, uint64_t scratchBytes,
                                      hulk_index_search_stats *stats) const {
        hulk_index_search_opts o = hulk_index_search_opts();
        o.k = k; o.flags = flags; o.max_distance = maxDistance; o.scratch_bytes = scratchBytes;
        const size_t kk = k ? k : 1;
        std::vector<uint32_t> index(M * kk + 1), count((size_t)M + 1);
        std::vector<double> distance(M * kk + 1);
        const int rc = hulk_index_search(h_, mins, M, &o, index.data(), distance.data(), count.data(), stats);
        if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
        std::vector<std::vector<Hit>> out(M);
        for (uint32_t i = 0; i < M; i++)
            for (uint32_t j = 0; j < count[i]; j++) { Hit h; h.Index = index[i * kk + j]; h.Distance = distance[i * kk + j]; out[i].push_back(h); }
        return out;
    }
    static std::vector<uint64_t> Pack(const std::vector<HistoSketch> &set, uint32_t S) {
        std::vector<uint64_t> mins(set.size() * (size_t)S + 1);
        for (size_t i = 0; i < set.size(); i++) {
            if (set[i].Sketch.size() != S)
                throw Error(HULK_ERR_ARG, "sketch length mismatch: " + std::to_string(set[i].Sketch.size()) + " vs " + std::to_string(S) + "\n");
            std::copy(set[i].Sketch.begin(), set[i].Sketch.end(), mins.begin() + i * (size_t)S);
        }
        return mins;
    }
    hulk_index *h_ = nullptr;
};

// Single-linkage clusters of a collection at a distance threshold, on the GPU (hulk_cluster): sketches i != j are linked when Smash's
// entry [i][j] or [j][i] is <= maxDistance (in [0, 1]; a NaN never links, equality does); a cluster is a connected component, the
// label of a sketch the smallest index in its cluster.  bandRows (a multiple of 32, 0 = default) cannot change the result.
inline std::vector<uint32_t> Cluster(const std::vector<HistoSketch> &sketches, double maxDistance, const std::string &metric,
                                     uint32_t bandRows = 0, int device = 0, hulk_cluster_stats *stats = nullptr) {
    const uint32_t N = (uint32_t)sketches.size(), S = N ? sketches[0].SketchSize : 0;
    std::vector<uint64_t> mins;
    std::vector<double> weights;
    detail::Pack(sketches, mins, weights);
    hulk_cluster_opts o = hulk_cluster_opts();
    o.max_distance = maxDistance; o.band_rows = bandRows;
    o.metric = MetricCode(metric);
    std::vector<uint32_t> label((size_t)N + 1);
    const int rc = hulk_cluster(device, mins.data(), weights.data(), N, S, &o, label.data(), stats);
    if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
    label.resize(N);
    return label;
}

// The directory form (hulk_cluster_files): the files through the library's loader (sorted unique paths, the reference's error
// texts), the labels in that order; clustersCSV, if not empty, receives "sketch,cluster,size,representative".
inline std::vector<uint32_t> ClusterFiles(const std::vector<std::string> &jsonFiles, uint32_t kSize, const std::string &algo,
                                          const std::string &metric, double maxDistance, const std::string &clustersCSV = std::string(),
                                          hulk_cluster_stats *stats = nullptr, int device = 0, uint32_t threads = 0) {
    const std::vector<const char *> ptr = detail::CPaths(jsonFiles);
    const std::vector<std::string> uniq = detail::SortedUnique(jsonFiles);
    std::vector<uint32_t> label(uniq.size() + 1);
    char err[4096] = {0};
    const int rc = hulk_cluster_files(device, ptr.data(), (uint32_t)ptr.size(), kSize, algo.c_str(), metric.c_str(), maxDistance, threads,
                                      clustersCSV.empty() ? nullptr : clustersCSV.c_str(), label.data(), stats, err, sizeof err);
    if (rc != HULK_OK) throw Error(rc, err);
    label.resize(uniq.size());
    return label;
}

// The links of a collection as a sparse graph, on the GPU (hulk_links): row i lists every j != i whose Smash entry [i][j] is <=
// maxDistance (in [0, 1]; a NaN never is listed, equality is) in ascending j, with that entry bit for bit.  CSR: the edges of row i
// are Indices / Distances [RowStart[i], RowStart[i + 1]).  weightedjaccard is directed; upper keeps j > i only; without it every
// metric pays the full square.  maxEdges (0 = none): more edges than that throws (HULK_ERR_ARG; the text names the cap and the count).
// The struct owns the library's list and frees it; the three pointers are valid while it lives.
struct LinkList {
    uint32_t N = 0;
    uint64_t Edges = 0;
    const uint64_t *RowStart = nullptr;    // [N + 1]
    const uint32_t *Indices = nullptr;     // [Edges]
    const double *Distances = nullptr;     // [Edges]
    LinkList() = default;
    explicit LinkList(hulk_link_list *list) : list_(list) {
        hulk_link_list_info(list, &N, &Edges);
        RowStart = hulk_link_list_row_start(list); Indices = hulk_link_list_cols(list); Distances = hulk_link_list_distances(list);
    }
    LinkList(LinkList &&o) noexcept { *this = std::move(o); }
    LinkList &operator=(LinkList &&o) noexcept {
        if (this != &o) {
            hulk_link_list_free(list_);
            list_ = o.list_; N = o.N; Edges = o.Edges; RowStart = o.RowStart; Indices = o.Indices; Distances = o.Distances;
            o.list_ = nullptr; o.N = 0; o.Edges = 0; o.RowStart = nullptr; o.Indices = nullptr; o.Distances = nullptr;
        }
        return *this;
    }
    LinkList(const LinkList &) = delete;
    LinkList &operator=(const LinkList &) = delete;
    ~LinkList() { hulk_link_list_free(list_); }

  private:
    hulk_link_list *list_ = nullptr;
};
inline LinkList Links(const std::vector<HistoSketch> &sketches, double maxDistance, const std::string &metric, bool upper = false,
                      uint64_t maxEdges = 0, uint32_t bandRows = 0, int device = 0, hulk_links_stats *stats = nullptr) {
    const uint32_t N = (uint32_t)sketches.size(), S = N ? sketches[0].SketchSize : 0;
    std::vector<uint64_t> mins;
    std::vector<double> weights;
    detail::Pack(sketches, mins, weights);
    hulk_links_opts o = hulk_links_opts();
    o.max_distance = maxDistance; o.band_rows = bandRows; o.flags = upper ? HULK_LINKS_UPPER : 0u; o.max_edges = maxEdges;
    o.metric = MetricCode(metric);
    hulk_link_list *list = nullptr;
    const int rc = hulk_links(device, mins.data(), weights.data(), N, S, &o, &list, stats);
    if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
    return LinkList(list);
}

// The directory form (hulk_links_files): the files through the library's loader (sorted unique paths, which the rows and indices
// count; the reference's error texts); linksCSV, if not empty, receives "sketch,neighbour,distance,similarity", one line per edge.
inline LinkList LinksFiles(const std::vector<std::string> &jsonFiles, uint32_t kSize, const std::string &algo, const std::string &metric,
                           double maxDistance, bool upper = false, uint64_t maxEdges = 0, const std::string &linksCSV = std::string(),
                           hulk_links_stats *stats = nullptr, int device = 0, uint32_t threads = 0) {
    const std::vector<const char *> ptr = detail::CPaths(jsonFiles);
    char err[4096] = {0};
    hulk_link_list *list = nullptr;
    const int rc = hulk_links_files(device, ptr.data(), (uint32_t)ptr.size(), kSize, algo.c_str(), metric.c_str(), maxDistance,
                                    upper ? HULK_LINKS_UPPER : 0u, maxEdges, threads, linksCSV.empty() ? nullptr : linksCSV.c_str(), &list, stats,
                                    err, sizeof err);
    if (rc != HULK_OK) throw Error(rc, err);
    return LinkList(list);
}

// The single-linkage dendrogram of a collection, on the GPU (hulk_dendrogram): the minimum spanning forest of the graph whose edge
// {i, j} weighs fmin(Smash's [i][j], [j][i]) (NaNs ignored; two NaNs: no edge), edges ordered by (weight, A, B): A < B, ascending —
// the merge order.  Cut at any distance it is hulk::Cluster at that maxDistance.  bandRows cannot change the result.
struct DendrogramEdge { uint32_t A = 0, B = 0; double Distance = 0; };
inline std::vector<DendrogramEdge> Dendrogram(const std::vector<HistoSketch> &sketches, const std::string &metric, uint32_t bandRows = 0,
                                              int device = 0, hulk_dendrogram_stats *stats = nullptr) {
    const uint32_t N = (uint32_t)sketches.size(), S = N ? sketches[0].SketchSize : 0;
    std::vector<uint64_t> mins;
    std::vector<double> weights;
    detail::Pack(sketches, mins, weights);
    hulk_dendrogram_opts o = hulk_dendrogram_opts();
    o.band_rows = bandRows;
    o.metric = MetricCode(metric);
    std::vector<uint32_t> a((size_t)N + 1), b((size_t)N + 1);
    std::vector<double> d((size_t)N + 1);
    uint32_t m = 0;
    const int rc = hulk_dendrogram(device, mins.data(), weights.data(), N, S, &o, a.data(), b.data(), d.data(), &m, stats);
    if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
    std::vector<DendrogramEdge> out(m);
    for (uint32_t e = 0; e < m; e++) { out[e].A = a[e]; out[e].B = b[e]; out[e].Distance = d[e]; }
    return out;
}

// The directory form (hulk_dendrogram_files): the files through the library's loader (sorted unique paths, which A and B count);
// dendrogramCSV, if not empty, receives "merge,sketch_a,sketch_b,distance,similarity,size"; cutDistance in [0, 1] (NaN: no cut)
// with clustersCSV: the file hulk::ClusterFiles writes at that maxDistance.
inline std::vector<DendrogramEdge> DendrogramFiles(const std::vector<std::string> &jsonFiles, uint32_t kSize, const std::string &algo,
                                                   const std::string &metric, const std::string &dendrogramCSV = std::string(),
                                                   double cutDistance = std::numeric_limits<double>::quiet_NaN(),
                                                   const std::string &clustersCSV = std::string(), hulk_dendrogram_stats *stats = nullptr,
                                                   int device = 0, uint32_t threads = 0) {
    const std::vector<const char *> ptr = detail::CPaths(jsonFiles);
    const size_t n = jsonFiles.size() + 1;
    std::vector<uint32_t> a(n), b(n);
    std::vector<double> d(n);
    uint32_t m = 0;
    char err[4096] = {0};
    const int rc = hulk_dendrogram_files(device, ptr.data(), (uint32_t)ptr.size(), kSize, algo.c_str(), metric.c_str(), threads,
                                         dendrogramCSV.empty() ? nullptr : dendrogramCSV.c_str(), cutDistance,
                                         clustersCSV.empty() ? nullptr : clustersCSV.c_str(), a.data(), b.data(), d.data(), &m, stats, err, sizeof err);
    if (rc != HULK_OK) throw Error(rc, err);
    std::vector<DendrogramEdge> out(m);
    for (uint32_t e = 0; e < m; e++) { out[e].A = a[e]; out[e].B = b[e]; out[e].Distance = d[e]; }
    return out;
}

// The dendrogram of a collection under "single", "complete" or "average" linkage, on the GPU (hulk_linkage): the agglomeration over
// W = fmin(Smash's [i][j], [j][i]) (two NaNs: +inf, never merged); clusters are named by their smallest member and the pair (A, B),
// A < B, smallest under (distance, A, B) merges into A.  The merges come in the order performed; Size: the members of the union.
struct LinkageMerge { uint32_t A = 0, B = 0; double Distance = 0; uint32_t Size = 0; };
inline int LinkageCode(const std::string &method) {
    if (method == "single") return HULK_LINKAGE_SINGLE;
    if (method == "complete") return HULK_LINKAGE_COMPLETE;
    if (method == "average") return HULK_LINKAGE_AVERAGE;
    throw Error(HULK_ERR_ARG, "supplied linkage is not available: " + method + "\nplease select one of the following: [single complete average]");
}
inline std::vector<LinkageMerge> Linkage(const std::vector<HistoSketch> &sketches, const std::string &method, const std::string &metric,
                                         int device = 0, hulk_linkage_stats *stats = nullptr) {
    const uint32_t N = (uint32_t)sketches.size(), S = N ? sketches[0].SketchSize : 0;
    std::vector<uint64_t> mins;
    std::vector<double> weights;
    detail::Pack(sketches, mins, weights);
    hulk_linkage_opts o = hulk_linkage_opts();
    o.method = LinkageCode(method);
    o.metric = MetricCode(metric);
    std::vector<uint32_t> a((size_t)N + 1), b((size_t)N + 1), s((size_t)N + 1);
    std::vector<double> d((size_t)N + 1);
    uint32_t m = 0;
    const int rc = hulk_linkage(device, mins.data(), weights.data(), N, S, &o, a.data(), b.data(), d.data(), s.data(), &m, stats);
    if (rc != HULK_OK) throw Error(rc, hulk_last_error(nullptr));
    std::vector<LinkageMerge> out(m);
    for (uint32_t e = 0; e < m; e++) { out[e].A = a[e]; out[e].B = b[e]; out[e].Distance = d[e]; out[e].Size = s[e]; }
    return out;
}

// The directory form (hulk_linkage_files): DendrogramFiles' loader, files and cut under the linkage `method`.
inline std::vector<LinkageMerge> LinkageFiles(const std::vector<std::string> &jsonFiles, uint32_t kSize, const std::string &algo,
                                              const std::string &metric, const std::string &method, const std::string &dendrogramCSV = std::string(),
                                              double cutDistance = std::numeric_limits<double>::quiet_NaN(),
                                              const std::string &clustersCSV = std::string(), hulk_linkage_stats *stats = nullptr,
                                              int device = 0, uint32_t threads = 0) {
    const std::vector<const char *> ptr = detail::CPaths(jsonFiles);
    const size_t n = jsonFiles.size() + 1;
    std::vector<uint32_t> a(n), b(n), s(n);
    std::vector<double> d(n);
    uint32_t m = 0;
    char err[4096] = {0};
    const int rc = hulk_linkage_files(device, ptr.data(), (uint32_t)ptr.size(), kSize, algo.c_str(), metric.c_str(), method.c_str(), threads,
                                      dendrogramCSV.empty() ? nullptr : dendrogramCSV.c_str(), cutDistance,
                                      clustersCSV.empty() ? nullptr : clustersCSV.c_str(), a.data(), b.data(), d.data(), s.data(), &m, stats, err, sizeof err);
    if (rc != HULK_OK) throw Error(rc, err);
    std::vector<LinkageMerge> out(m);
    for (uint32_t e = 0; e < m; e++) { out[e].A = a[e]; out[e].B = b[e]; out[e].Distance = d[e]; out[e].Size = s[e]; }
    return out;
}

// `hulk smash` as the reference runs it (cmd/smash.go:160-226): the sketch files of a directory in, <outFile>.hulk-matrix.csv out —
// LoadHULKdata (JSON, class / version, MD5) for every file, FindSketch(kSize, algo), the matrix on the GPU, the CSV — all inside the
// library (hulk_smash_files).  Returns the distances in sorted-path order, [s * N + q]; throws hulk::Error with the reference's message.
struct SmashStats { double SecondsLoad = 0, SecondsMatrix = 0, SecondsCSV = 0, KernelMs = 0; uint32_t Sketches = 0, SketchSize = 0; };
inline std::vector<double> SmashFiles(const std::vector<std::string> &jsonFiles, uint32_t kSize, const std::string &algo,
                                      const std::string &metric, const std::string &matrixCSV, const std::string &bannerCSV = std::string(),
                                      SmashStats *stats = nullptr, int device = 0, uint32_t threads = 0) {
    const std::vector<const char *> ptr = detail::CPaths(jsonFiles);
    const std::vector<std::string> uniq = detail::SortedUnique(jsonFiles);
    std::vector<double> out(uniq.size() * uniq.size());
    hulk_smash_stats st;
    char err[4096] = {0};
    const int rc = hulk_smash_files(device, ptr.data(), (uint32_t)ptr.size(), kSize, algo.c_str(), metric.c_str(), threads,
                                    matrixCSV.empty() ? nullptr : matrixCSV.c_str(), bannerCSV.empty() ? nullptr : bannerCSV.c_str(),
                                    out.data(), &st, err, sizeof err);
    if (rc != HULK_OK) throw Error(rc, err);
    if (stats) *stats = SmashStats{st.seconds_load, st.seconds_matrix, st.seconds_csv, st.kernel_ms, st.n_sketches, st.sketch_size};
    return out;
}

}  // namespace hulk
#endif
