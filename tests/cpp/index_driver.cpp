// Drives hulk::Index of the C++ host mirror (include/hulk.hpp) for tests/test_gpu_index.py to compare with the ctypes path.
//   index_driver <queries.txt|-> <database.txt> S k buildDistance bands maxDistance scratchBytes <file.hulk-index>
// The text files: one sketch per line, S mins (decimal); "-" for the queries searches the indexed sketches among themselves.  Builds,
// searches, saves, loads the file and searches again: prints "info <n> <S> <bands> <device bytes>", one line per query
// "<query> <count> <index>:<distance> ..." (the distances as %a) from the built index, "stats <candidates> <within>" and
// "loaded <1|0>": whether the loaded index gave the same hits.
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
        out.push_back(hs);
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc < 10) { std::fprintf(stderr, "usage: index_driver <queries.txt|-> <database.txt> S k buildDistance bands maxDistance scratchBytes <file>\n"); return 2; }
    try {
        const unsigned S = (unsigned)std::atoi(argv[3]);
        const bool self = std::string(argv[1]) == "-";
        std::vector<hulk::HistoSketch> queries;
        if (!self) queries = read_sketches(argv[1], S);
        const std::vector<hulk::HistoSketch> database = read_sketches(argv[2], S);
        const uint32_t k = (uint32_t)std::atoi(argv[4]);
        const double limit = std::atof(argv[7]);
        const uint64_t scratch = std::strtoull(argv[8], nullptr, 10);
        hulk::Index ix = hulk::Index::Build(database, std::atof(argv[5]), (uint32_t)std::atoi(argv[6]));
        std::printf("info %u %u %u %llu\n", ix.Size(), ix.SketchSize(), ix.Bands(), (unsigned long long)ix.DeviceBytes());
        hulk_index_search_stats st;
        const auto hits = self ? ix.SearchSelf(k, limit, scratch, &st) : ix.Search(queries, k, limit, scratch, &st);
        for (size_t i = 0; i < hits.size(); i++) {
            std::printf("%zu %zu", i, hits[i].size());
            for (const hulk::Hit &h : hits[i]) std::printf(" %u:%a", h.Index, h.Distance);
            std::printf("\n");
        }
        std::printf("stats %llu %llu\n", (unsigned long long)st.candidates, (unsigned long long)st.within);
        ix.Save(argv[9]);
        hulk::Index again = hulk::Index::Load(argv[9]);
        ix = std::move(again);                                      // (the built index is freed here)
        const auto hits2 = self ? ix.SearchSelf(k, limit, scratch) : ix.Search(queries, k, limit, scratch);
        bool same = hits.size() == hits2.size();
        for (size_t i = 0; same && i < hits.size(); i++) {
            same = hits[i].size() == hits2[i].size();
            for (size_t j = 0; same && j < hits[i].size(); j++) same = hits[i][j].Index == hits2[i][j].Index && hits[i][j].Distance == hits2[i][j].Distance;
        }
        std::printf("loaded %d\n", same ? 1 : 0);
        try {                                                       // no queries is an error, never a self-join
            ix.Search(std::vector<hulk::HistoSketch>(), k);
            std::printf("empty accepted\n");
        } catch (const hulk::Error &e) {
            std::printf("empty %d\n", e.code());
        }
        return 0;
    } catch (const hulk::Error &e) {
        std::printf("hulk::Error %d|%s\n", e.code(), e.what());
        return 1;
    }
}
