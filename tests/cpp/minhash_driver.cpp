// Drives the MinHash side of the C++ host mirror (include/hulk.hpp): a Boss created with SketchInfo.KMV / .KHF, fed one
// sequence per line of <reads.txt> through AddSeq, prints one JSON line with both signatures
// (tests/test_gpu_minhash.py compares it with the ctypes path and the numpy restatement of kmv.go / khf.go).
//   minhash_driver <reads.txt> k w S interval
//   minhash_driver noflag                       CollectKMVsketch on a Boss without the flag: the error's code and text
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "hulk.hpp"

static void print_list(const char *name, const std::vector<uint64_t> &v, const char *tail) {
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) std::printf("%s%llu", i ? ", " : "", (unsigned long long)v[i]);
    std::printf("]%s", tail);
}

int main(int argc, char **argv) {
    try {
        if (argc > 1 && std::string(argv[1]) == "noflag") {
            hulk::SketchInfo info; info.SketchSize = 8;
            hulk::Boss boss = hulk::Boss::FindMinimizers(info);
            try { boss.CollectKMVsketch(); std::printf("no error\n"); }
            catch (const hulk::Error &e) { std::printf("%d|%s\n", e.code(), e.what()); }
            return 0;
        }
        if (argc < 6) { std::fprintf(stderr, "usage: minhash_driver <reads.txt> k w S interval | noflag\n"); return 2; }
        hulk::SketchInfo info;
        info.KmerSize = (unsigned)std::atoi(argv[2]); info.WindowSize = (unsigned)std::atoi(argv[3]);
        info.SketchSize = (unsigned)std::atoi(argv[4]); info.Interval = (unsigned)std::atoi(argv[5]);
        info.KMV = true; info.KHF = true;
        hulk::Boss theBoss = hulk::Boss::FindMinimizers(info);
        std::ifstream in(argv[1]);
        std::string line;
        uint64_t seqCount = 0;
        while (std::getline(in, line)) {
            if (line.empty()) continue;
            theBoss.AddSeq(line);
            seqCount++;
        }
        theBoss.StopWork();
        std::printf("{\"n_seqs\": %llu, \"n_minimizers\": %llu, ", (unsigned long long)seqCount,
                    (unsigned long long)theBoss.GetMinimizerCount());
        print_list("kmv", theBoss.CollectKMVsketch(), ", ");
        print_list("khf", theBoss.CollectKHFsketch(), "}\n");
        return 0;
    } catch (const hulk::Error &e) {
        std::fprintf(stderr, "ERROR---> %s\n", e.what());
        return 1;
    }
}
