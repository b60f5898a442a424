// Drives hulk::Search of the C++ host mirror (include/hulk.hpp) for tests/test_gpu_search.py to compare with the ctypes path.
//   search_driver <queries.txt> <database.txt|-> S k metric row|column maxDistance scratchBytes
// <queries.txt> / <database.txt>: one sketch per line, S mins (decimal) then S weights (%a or decimal); "-" for the database
// searches the queries among themselves.  Prints one line per query, "<query> <count> <index>:<distance> ...", the distances as %a
// (bit-exact), then "stats <strips> <query blocks>".
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
    if (argc < 9) { std::fprintf(stderr, "usage: search_driver <queries.txt> <database.txt|-> S k metric row|column maxDistance scratchBytes\n"); return 2; }
    try {
        const unsigned S = (unsigned)std::atoi(argv[3]);
        const std::vector<hulk::HistoSketch> queries = read_sketches(argv[1], S);
        std::vector<hulk::HistoSketch> database;
        if (std::string(argv[2]) != "-") database = read_sketches(argv[2], S);
        hulk_search_stats st;
        const auto hits = hulk::Search(queries, database, (uint32_t)std::atoi(argv[4]), argv[5], std::string(argv[6]) == "row", std::atof(argv[7]),
                                       std::strtoull(argv[8], nullptr, 10), 0, &st);
        for (size_t i = 0; i < hits.size(); i++) {
            std::printf("%zu %zu", i, hits[i].size());
            for (const hulk::Hit &h : hits[i]) std::printf(" %u:%a", h.Index, h.Distance);
            std::printf("\n");
        }
        std::printf("stats %u %u\n", st.strips, st.query_blocks);
        return 0;
    } catch (const hulk::Error &e) {
        std::printf("hulk::Error %d|%s\n", e.code(), e.what());
        return 1;
    }
}
