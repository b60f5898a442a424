// Drives hulk::Dendrogram of the C++ host mirror (include/hulk.hpp) for tests/test_gpu_dendrogram.py to compare with the ctypes path.
//   dendrogram_driver <sketches.txt> S metric bandRows
// <sketches.txt>: one sketch per line, S mins (decimal) then S weights (%a or decimal).  Prints one line "edge <a> <b> <distance as %a>"
// per edge in merge order, then "stats <rounds> <bands> <edges> <components>".
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
    if (argc < 5) { std::fprintf(stderr, "usage: dendrogram_driver <sketches.txt> S metric bandRows\n"); return 2; }
    try {
        const unsigned S = (unsigned)std::atoi(argv[2]);
        const std::vector<hulk::HistoSketch> sketches = read_sketches(argv[1], S);
        hulk_dendrogram_stats st;
        const std::vector<hulk::DendrogramEdge> edges = hulk::Dendrogram(sketches, argv[3], (uint32_t)std::strtoul(argv[4], nullptr, 10), 0, &st);
        for (const hulk::DendrogramEdge &e : edges) std::printf("edge %u %u %a\n", e.A, e.B, e.Distance);
        std::printf("stats %u %u %u %u\n", st.rounds, st.bands, st.edges, st.components);
        return 0;
    } catch (const hulk::Error &e) {
        std::printf("hulk::Error %d|%s\n", e.code(), e.what());
        return 1;
    }
}
