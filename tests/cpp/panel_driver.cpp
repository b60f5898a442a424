// Drives the panel side of the C++ host mirror (include/hulk.hpp): a Boss with EnableSnapshots and SetPanel, fed one sequence
// per line of <reads.txt> through AddSeq, prints one line per snapshot — "<ordinal> <n_reads> <distance> ..." with the distances
// as %a (bit-exact) — for tests/test_gpu_panel.py to compare with the ctypes path.  <panel.txt>: one sketch per line, S mins
// (decimal) then S weights (%a or decimal).
//   panel_driver collect  <reads.txt> <panel.txt> k w S interval decay every capacity metric row|column    Boss::CollectSnapshots
//   panel_driver callback <reads.txt> <panel.txt> k w S interval decay every capacity metric row|column    Boss::OnSnapshot
//   panel_driver moved    ...      collect, through a Boss that was MOVED after SetPanel (into a std::optional, as a host that keeps it in a member would)
//   panel_driver reenable ...      collect, after EnableSnapshots was called again behind SetPanel: the panel is gone, Distances are empty
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "hulk.hpp"

static void print_snapshot(const hulk::Snapshot &s) {
    std::printf("%llu %llu", (unsigned long long)s.Ordinal, (unsigned long long)s.Reads);
    for (double d : s.Distances) std::printf(" %a", d);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 13) { std::fprintf(stderr, "usage: panel_driver collect|callback|moved|reenable <reads.txt> <panel.txt> k w S interval decay every capacity metric row|column\n"); return 2; }
    const std::string mode = argv[1];
    try {
        hulk::SketchInfo info;
        info.KmerSize = (unsigned)std::atoi(argv[4]); info.WindowSize = (unsigned)std::atoi(argv[5]);
        info.SketchSize = (unsigned)std::atoi(argv[6]); info.Interval = (unsigned)std::atoi(argv[7]);
        info.DecayRatio = std::atof(argv[8]);
        std::vector<hulk::HistoSketch> panel;
        {
            std::ifstream in(argv[3]);
            std::string line;
            while (std::getline(in, line)) {
                if (line.empty()) continue;
                std::istringstream ss(line);
                hulk::HistoSketch hs;
                hs.KmerSize = info.KmerSize; hs.SketchSize = info.SketchSize;
                std::string tok;
                for (unsigned i = 0; i < info.SketchSize && (ss >> tok); i++) hs.Sketch.push_back(std::strtoull(tok.c_str(), nullptr, 10));
                for (unsigned i = 0; i < info.SketchSize && (ss >> tok); i++) hs.SketchWeights.push_back(std::strtod(tok.c_str(), nullptr));
                panel.push_back(hs);
            }
        }
        hulk::Boss first = hulk::Boss::FindMinimizers(info);
        first.EnableSnapshots((uint32_t)std::atoi(argv[9]), (uint32_t)std::atoi(argv[10]));
        first.SetPanel(panel, argv[11], std::string(argv[12]) == "row");
        if (mode == "reenable") first.EnableSnapshots((uint32_t)std::atoi(argv[9]), (uint32_t)std::atoi(argv[10]));
        std::optional<hulk::Boss> held;
        if (mode == "moved") held.emplace(std::move(first));
        hulk::Boss &theBoss = held ? *held : first;
        unsigned seen = 0;
        if (mode == "callback") theBoss.OnSnapshot([&](const hulk::Snapshot &s) { seen++; print_snapshot(s); });
        std::ifstream in(argv[2]);
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty()) continue;
            theBoss.AddSeq(line);
        }
        theBoss.StopWork();
        if (mode != "callback") for (const hulk::Snapshot &s : theBoss.CollectSnapshots()) print_snapshot(s);
        std::printf("final %u\n", seen);
        return 0;
    } catch (const hulk::Error &e) {
        std::printf("hulk::Error %d|%s\n", e.code(), e.what());
        return 1;
    }
}
