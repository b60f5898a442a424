// bottomk_host.cpp — hulk_amd/csrc/hulk_bottomk_merge.h compiled for the host (tests/test_bottomk_cpu.py builds it with
// -fsanitize=address,undefined): the sorting network of k_bottomk_prep at every length, the run-length merge against the
// map-and-decrement loop of KMVsketch.GetSimilarity (kmv.go:143-156), and the tile's walk — windows of W entries a list, cut at the
// smallest last entry of the lists that go on — against the merge of the whole lists.  Prints "<check>: ok" or "<check>: FAILED".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

#define HULK_BK_FN static inline
#include "hulk_bottomk_merge.h"

typedef std::vector<uint64_t> List;

static List draw(std::mt19937_64 &rng, size_t n, uint64_t range) {
    List v(n);
    for (auto &x : v) {
        const uint64_t r = rng();
        x = r % 17 == 0 ? ~0ull : r % 19 == 0 ? 0ull : range ? r % range : r;       // the ends of uint64 are values like any other
    }
    return v;
}

// k_bottomk_prep's loop, one comparator at a time
static void net_sort(List &v) {
    const uint32_t S = (uint32_t)v.size();
    uint32_t p2 = 1;
    while (p2 < S) p2 <<= 1;
    for (uint32_t k = 2; k <= p2; k <<= 1)
        for (uint32_t j = 0;;) {
            for (uint32_t t = 0; t < p2 / 2; t++) {
                uint32_t lo, hi;
                bottomk_net_pair(t, k, j, &lo, &hi);
                if (hi < S && v[hi] < v[lo]) std::swap(v[lo], v[hi]);
            }
            j = j ? j >> 1 : k >> 2;
            if (!j) break;
        }
}

struct Rle { List val; std::vector<uint32_t> mult; };
static Rle rle(List v) {
    net_sort(v);
    Rle r;
    for (size_t i = 0; i < v.size(); i++) {
        if (i == 0 || v[i] != v[i - 1]) { r.val.push_back(v[i]); r.mult.push_back(0); }
        r.mult.back()++;
    }
    return r;
}

static uint32_t go_intersect(const List &a, const List &b) {         // kmv.go:143-156
    std::map<uint64_t, int> minimums;
    for (uint64_t v : a) minimums[v]++;
    uint32_t intersect = 0;
    for (uint64_t m : b) {
        auto it = minimums.find(m);
        if (it != minimums.end() && it->second > 0) { it->second--; intersect++; }
    }
    return intersect;
}

// the tile's rounds over `lists` with windows of W entries: cnt[a][b] for every pair
static std::vector<std::vector<uint32_t>> windowed(const std::vector<Rle> &lists, uint32_t W, uint32_t *rounds) {
    const size_t L = lists.size();
    std::vector<uint32_t> cur(L, 0), n(L, 0);
    std::vector<std::vector<uint32_t>> cnt(L, std::vector<uint32_t>(L, 0));
    *rounds = 0;
    for (;;) {
        uint64_t pivot = ~0ull;
        bool more = false;
        for (size_t l = 0; l < L; l++)
            if (cur[l] + W < lists[l].val.size()) { more = true; pivot = std::min(pivot, lists[l].val[cur[l] + W - 1]); }
        for (size_t l = 0; l < L; l++) {
            const uint32_t left = (uint32_t)lists[l].val.size() - cur[l], take = left < W ? left : W;
            // (a copy of exactly the window: the sanitizer sees a read behind it)
            const List win(lists[l].val.begin() + cur[l], lists[l].val.begin() + cur[l] + take);
            n[l] = bottomk_upto(win.data(), take, pivot);
        }
        for (size_t a = 0; a < L; a++)
            for (size_t b = 0; b < L; b++)
                cnt[a][b] += bottomk_merge(lists[a].val.data() + cur[a], lists[a].mult.data() + cur[a], n[a],
                                           lists[b].val.data() + cur[b], lists[b].mult.data() + cur[b], n[b]);
        for (size_t l = 0; l < L; l++) cur[l] += n[l];
        ++*rounds;
        if (!more) break;
    }
    for (size_t l = 0; l < L; l++) if (cur[l] != lists[l].val.size()) cnt[0][0] = ~0u;   // every list must end consumed
    return cnt;
}

static bool report(const char *name, bool ok) { printf("%s: %s\n", name, ok ? "ok" : "FAILED"); return ok; }

int main() {
    std::mt19937_64 rng(20240607);
    bool all = true;
    {   // the network sorts every length, duplicates and the ends of uint64 included
        bool ok = true;
        std::vector<size_t> lens;
        for (size_t n = 1; n <= 130; n++) lens.push_back(n);
        for (size_t n : {255, 256, 257, 511, 512, 513, 1000, 2047, 2048, 2049, 4095, 4096}) lens.push_back(n);
        for (size_t n : lens)
            for (uint64_t range : {0ull, 5ull, 1000ull}) {
                List v = draw(rng, n, range), w = v;
                net_sort(v);
                std::sort(w.begin(), w.end());
                ok = ok && v == w;
            }
        all &= report("sorting network, every length", ok);
    }
    {   // run-length merge = the map-and-decrement loop, both ways round
        bool ok = true;
        for (int rep = 0; rep < 400; rep++) {
            const size_t n = 1 + rng() % 300;
            const uint64_t range = rep % 3 == 0 ? 4 : rep % 3 == 1 ? n : 3 * n;
            const List a = draw(rng, n, range), b = draw(rng, n, range);
            const Rle ra = rle(a), rb = rle(b);
            const uint32_t got = bottomk_merge(ra.val.data(), ra.mult.data(), (uint32_t)ra.val.size(), rb.val.data(), rb.mult.data(), (uint32_t)rb.val.size());
            ok = ok && got == go_intersect(a, b) && got == go_intersect(b, a);
            uint32_t total = 0;
            for (uint32_t m : ra.mult) total += m;
            ok = ok && total == n && std::is_sorted(ra.val.begin(), ra.val.end()) && std::adjacent_find(ra.val.begin(), ra.val.end()) == ra.val.end();
        }
        all &= report("run-length merge against kmv.go's loop", ok);
    }
    {   // bottomk_upto at every pivot around every entry
        bool ok = true;
        const List v = {0, 3, 4, 9, ~0ull - 1};
        for (uint32_t n = 0; n <= v.size(); n++)
            for (uint64_t p : {0ull, 1ull, 3ull, 4ull, 5ull, 9ull, 10ull, ~0ull - 1, ~0ull}) {
                uint32_t want = 0;
                for (uint32_t i = 0; i < n; i++) want += v[i] <= p;
                ok = ok && bottomk_upto(v.data(), n, p) == want;
            }
        all &= report("entries up to a pivot", ok);
    }
    for (uint32_t W : {1u, 2u, 32u}) {   // the tile's rounds = the merge of the whole lists
        bool ok = true;
        for (int rep = 0; rep < 12; rep++) {
            const size_t L = 7, n = rep < 2 ? 1 : 20 + rng() % 200;
            std::vector<List> raw;
            std::vector<Rle> lists;
            for (size_t l = 0; l < L; l++) {
                // like densities, very different densities, long runs, one list all equal
                const uint64_t range = rep % 4 == 0 ? 2 * n : rep % 4 == 1 ? (l + 1) * (l + 1) * n : rep % 4 == 2 ? 6 : 0;
                raw.push_back(l == 3 && rep % 2 ? List(n, 5) : draw(rng, n, range));
                lists.push_back(rle(raw.back()));
            }
            uint32_t rounds = 0;
            const auto cnt = windowed(lists, W, &rounds);
            for (size_t a = 0; a < L; a++)
                for (size_t b = 0; b < L; b++) ok = ok && cnt[a][b] == go_intersect(raw[a], raw[b]);
            ok = ok && rounds <= L * (n / W + 1) + 1;              // one list at least consumes a whole window a round
        }
        char name[64];
        snprintf(name, sizeof name, "windows of %u entries", W);
        all &= report(name, ok);
    }
    return all ? 0 : 1;
}
