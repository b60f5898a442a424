// Drives hulk::Linkage of the C++ host mirror (include/hulk.hpp) for tests/test_gpu_linkage.py to compare with the ctypes path.
//   linkage_driver <sketches.txt> S metric method
// <sketches.txt>: one sketch per line, S mins (decimal) then S weights (%a or decimal).  Prints one line
// "merge <a> <b> <distance as %a> <size>" per merge in the order performed, then "stats <merges> <components> <rows_rescanned>".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "hulk.hpp"

static std::vector<hulk::HistoSketch> read_sketches(const char *path, unsigned S) {
    std::vector<hulk::HistoSketch> out;
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        hulk::HistoSketch hs;
        hs.SketchSize = S;
        std::string tok;
        for (unsigned i = 0; i < S && (ss >> tok); i++) hs.Sketch.push_back(std::strtoull(tok.c_str(), nullptr, 10));
        for (unsigned i = 0; i < S && (ss >> tok); i++) hs.SketchWeights.push_back(std::strtod(tok.c_str(), nullptr));
        out.push_back(hs);
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: linkage_driver <sketches.txt> S metric method\n"); return 2; }
    try {
        const unsigned S = (unsigned)std::atoi(argv[2]);
        const std::vector<hulk::HistoSketch> sketches = read_sketches(argv[1], S);
        hulk_linkage_stats st;
        const std::vector<hulk::LinkageMerge> merges = hulk::Linkage(sketches, argv[4], argv[3], 0, &st);
        for (const hulk::LinkageMerge &m : merges) std::printf("merge %u %u %a %u\n", m.A, m.B, m.Distance, m.Size);
        std::printf("stats %u %u %llu\n", st.merges, st.components, (unsigned long long)st.rows_rescanned);
        return 0;
    } catch (const hulk::Error &e) {
        std::printf("hulk::Error %d|%s\n", e.code(), e.what());
        return 1;
    }
}
