// Drives the snapshot side of the C++ host mirror (include/hulk.hpp): a Boss with EnableSnapshots, fed one sequence per line
// of <reads.txt> through AddSeq, prints one JSON line per snapshot — {"ordinal", "n_reads", "mins", "weights"} — and a last line
// with the final sketch (tests/test_gpu_snapshots.py compares them with the ctypes path).
//   snapshot_driver collect  <reads.txt> k w S interval decay every capacity     Boss::CollectSnapshots after StopWork
//   snapshot_driver callback <reads.txt> k w S interval decay every capacity     Boss::OnSnapshot, printed as they are delivered
//   snapshot_driver throw    <reads.txt> k w S interval decay every capacity     the function throws at the third snapshot
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>

#include "hulk.hpp"

static void print_sketch(const hulk::HistoSketch &hs) {
    std::printf("\"mins\": [");
    for (size_t i = 0; i < hs.Sketch.size(); i++) std::printf("%s%llu", i ? ", " : "", (unsigned long long)hs.Sketch[i]);
    std::printf("], \"weights\": [");
    for (size_t i = 0; i < hs.SketchWeights.size(); i++) std::printf("%s%.17g", i ? ", " : "", hs.SketchWeights[i]);
    std::printf("]");
}
static void print_snapshot(const hulk::Snapshot &s) {
    std::printf("{\"ordinal\": %llu, \"n_reads\": %llu, \"ksize\": %u, \"bins\": %d, \"drift\": %s, ", (unsigned long long)s.Ordinal,
                (unsigned long long)s.Reads, s.Sketch.KmerSize, (int)s.Sketch.Dimensions, s.Sketch.ApplyConceptDrift ? "true" : "false");
    print_sketch(s.Sketch);
    std::printf("}\n");
}

int main(int argc, char **argv) {
    if (argc < 10) { std::fprintf(stderr, "usage: snapshot_driver collect|callback|throw <reads.txt> k w S interval decay every capacity\n"); return 2; }
    const std::string mode = argv[1];
    try {
        hulk::SketchInfo info;
        info.KmerSize = (unsigned)std::atoi(argv[3]); info.WindowSize = (unsigned)std::atoi(argv[4]);
        info.SketchSize = (unsigned)std::atoi(argv[5]); info.Interval = (unsigned)std::atoi(argv[6]);
        info.DecayRatio = std::atof(argv[7]);
        hulk::Boss theBoss = hulk::Boss::FindMinimizers(info);
        theBoss.EnableSnapshots((uint32_t)std::atoi(argv[8]), (uint32_t)std::atoi(argv[9]));
        unsigned seen = 0;
        if (mode == "callback") theBoss.OnSnapshot([&](const hulk::Snapshot &s) { seen++; print_snapshot(s); });
        if (mode == "throw") theBoss.OnSnapshot([&](const hulk::Snapshot &) { if (++seen == 3) throw std::runtime_error("third snapshot"); });
        std::ifstream in(argv[2]);
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty()) continue;
            theBoss.AddSeq(line);
        }
        theBoss.StopWork();
        if (mode == "collect") for (const hulk::Snapshot &s : theBoss.CollectSnapshots()) print_snapshot(s);
        std::printf("{\"final\": true, \"delivered\": %u, ", seen);
        print_sketch(theBoss.Sketch());
        std::printf("}\n");
        return 0;
    } catch (const hulk::Error &e) {
        std::printf("hulk::Error %d|%s\n", e.code(), e.what());
        return 1;
    } catch (const std::runtime_error &e) {
        std::printf("runtime_error|%s|seen\n", e.what());
        return 3;
    }
}
