// Drives hulk::Links of the C++ host mirror (include/hulk.hpp) for tests/test_gpu_links.py to compare with the ctypes path.
//   links_driver <sketches.txt> S metric maxDistance upper maxEdges bandRows
// <sketches.txt>: one sketch per line, S mins (decimal) then S weights (%a or decimal); maxDistance as %a or decimal.  Prints
// "indptr <row_start[0]> ..", "indices <col[0]> ..", "distances <the bits of distance[0] in hex> ..", then
// "stats <edges> <bands> <max_degree>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    if (argc < 8) { std::fprintf(stderr, "usage: links_driver <sketches.txt> S metric maxDistance upper maxEdges bandRows\n"); return 2; }
    try {
        const unsigned S = (unsigned)std::atoi(argv[2]);
        const std::vector<hulk::HistoSketch> sketches = read_sketches(argv[1], S);
        hulk_links_stats st;
        hulk::LinkList moved;
        {
            hulk::LinkList got = hulk::Links(sketches, std::strtod(argv[4], nullptr), argv[3], std::atoi(argv[5]) != 0, std::strtoull(argv[6], nullptr, 10),
                                             (uint32_t)std::strtoul(argv[7], nullptr, 10), 0, &st);
            moved = std::move(got);                                 // (the moved-from struct frees nothing)
        }
        std::printf("indptr");
        for (uint32_t i = 0; i <= moved.N; i++) std::printf(" %llu", (unsigned long long)moved.RowStart[i]);
        std::printf("\nindices");
        for (uint64_t e = 0; e < moved.Edges; e++) std::printf(" %u", moved.Indices[e]);
        std::printf("\ndistances");
        for (uint64_t e = 0; e < moved.Edges; e++) { uint64_t bits; std::memcpy(&bits, &moved.Distances[e], 8); std::printf(" %llx", (unsigned long long)bits); }
        std::printf("\nstats %llu %u %u\n", (unsigned long long)st.edges, st.bands, st.max_degree);
        return 0;
    } catch (const hulk::Error &e) {
        std::printf("hulk::Error %d|%s\n", e.code(), e.what());
        return 1;
    }
}
