// Drives hulk::Cluster of the C++ host mirror (include/hulk.hpp) for tests/test_gpu_cluster.py to compare with the ctypes path.
//   cluster_driver <sketches.txt> S metric maxDistance bandRows
// <sketches.txt>: one sketch per line, S mins (decimal) then S weights (%a or decimal); maxDistance as %a or decimal.  Prints
// "labels <label of sketch 0> <label of sketch 1> ...", then "stats <links> <bands> <clusters>".
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
    if (argc < 6) { std::fprintf(stderr, "usage: cluster_driver <sketches.txt> S metric maxDistance bandRows\n"); return 2; }
    try {
        const unsigned S = (unsigned)std::atoi(argv[2]);
        const std::vector<hulk::HistoSketch> sketches = read_sketches(argv[1], S);
        hulk_cluster_stats st;
        const std::vector<uint32_t> label = hulk::Cluster(sketches, std::strtod(argv[4], nullptr), argv[3], (uint32_t)std::strtoul(argv[5], nullptr, 10), 0, &st);
        std::printf("labels");
        for (uint32_t l : label) std::printf(" %u", l);
        std::printf("\nstats %llu %u %u\n", (unsigned long long)st.links, st.bands, st.clusters);
        return 0;
    } catch (const hulk::Error &e) {
        std::printf("hulk::Error %d|%s\n", e.code(), e.what());
        return 1;
    }
}
