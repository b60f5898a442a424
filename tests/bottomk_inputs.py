"""The yardstick of the bottom-k metric (HULK_METRIC_BOTTOMK) and the inputs of its tests.

go_similarity is KMVsketch.GetSimilarity (src/minhash/kmv.go:136-158) restated line by line: longer / shorter, the map of counts, the
decrement.  distance = 1.0 - similarity, in Python floats (IEEE doubles: the expression the kernels evaluate).  matrix() computes all
pairs of a set another way — a value that occurs m times becomes the m keys (value, 0) .. (value, m - 1), and the multiset intersection
is the number of keys two sketches share — and holds itself to go_similarity, on every pair of a small set and on a sample of a
large one.  The tile's constants are read from the header, so that the planted runs sit where the code's boundaries are."""
import functools
import os
import re
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64_MAX = 2 ** 64 - 1


def go_similarity(a, b):
    a = [int(v) for v in a]; b = [int(v) for v in b]
    # assign longer and shorter heaps
    if len(a) > len(b):
        longer, shorter = a, b
    else:
        shorter, longer = a, b
    # make a map of one of the sketches, recording each unique minimum and its count
    minimums = {}
    for v in longer:
        minimums[v] = minimums.get(v, 0) + 1
    # iterate over the other sketch and calculate the intersect
    intersect = 0
    for minimum in shorter:
        count = minimums.get(minimum)
        if count is not None and count > 0:
            minimums[minimum] = count - 1
            intersect += 1
    return float(intersect) / float(len(longer))


def distance(a, b):
    return 1.0 - go_similarity(a, b)


def counter_similarity(a, b):
    """the same number from collections.Counter: what go_similarity is held to"""
    return sum((Counter(int(v) for v in a) & Counter(int(v) for v in b)).values()) / len(a)


def intersections(mins):
    """[n][n] multiset intersection counts of the rows of mins [n][S], through (value, occurrence) keys"""
    mins = np.ascontiguousarray(mins, dtype=np.uint64)
    n, s = mins.shape
    srt = np.sort(mins, axis=1)
    occ = np.zeros((n, s), dtype=np.int64)
    for c in range(1, s):
        occ[:, c] = np.where(srt[:, c] == srt[:, c - 1], occ[:, c - 1] + 1, 0)
    keys = np.empty(n * s, dtype=[("v", np.uint64), ("k", np.int64)])
    keys["v"] = srt.ravel(); keys["k"] = occ.ravel()
    _, ids = np.unique(keys, return_inverse=True)
    inc = np.zeros((n, int(ids.max()) + 1), dtype=np.float32)       # (a key occurs once in a row; counts <= 4096 are exact in fp32)
    inc[np.repeat(np.arange(n), s), ids.ravel()] = 1.0
    return np.rint(inc @ inc.T).astype(np.int64)


def matrix(mins, sample=300, seed=1):
    """the yardstick's [n][n] distances; checked against go_similarity pair by pair (all pairs of a small set, `sample` of a large one)"""
    mins = np.ascontiguousarray(mins, dtype=np.uint64)
    n, s = mins.shape
    cnt = intersections(mins)
    D = np.array([[1.0 - float(int(c)) / float(s) for c in row] for row in cnt], dtype=np.float64)
    pairs = [(i, j) for i in range(n) for j in range(n)]
    if n * n * s > 200000:
        rng = np.random.default_rng(seed)
        pairs = [pairs[k] for k in rng.choice(len(pairs), size=sample, replace=False)]
    for i, j in pairs:
        want = distance(mins[i], mins[j])
        assert D[i, j] == want, f"the yardstick's two forms differ at ({i}, {j}): {D[i, j]!r} vs {want!r}"
    return D


@functools.lru_cache(maxsize=None)
def tile_constants():
    """BK_W: entries of a list's window in the tile; PREP_THREADS: the threads that share a sketch's run heads in k_bottomk_prep;
    TS / TQ: the tile's subjects and others"""
    tile = open(os.path.join(ROOT, "hulk_amd", "csrc", "hulk_bottomk_tile.h")).read()
    prep = open(os.path.join(ROOT, "hulk_amd", "csrc", "hulk_bottomk.hip")).read()
    pair = open(os.path.join(ROOT, "hulk_amd", "csrc", "hulk_pairtile.h")).read()
    return dict(BK_W=int(re.search(r"constexpr int BK_W = (\d+)", tile).group(1)),
                PREP_THREADS=int(re.search(r"BK_PREP_THREADS = (\d+)", prep).group(1)),
                TS=int(re.search(r"PAIR_TS = (\d+)", pair).group(1)), TQ=int(re.search(r"PAIR_TQ = (\d+)", pair).group(1)))


def cat(*parts):
    """one uint64 list of the parts (never through int64 or float64: the values use all 64 bits)"""
    return np.concatenate([np.asarray(p, dtype=np.uint64).ravel() for p in parts])


def from_runs(values, mults):
    return np.repeat(np.asarray(values, dtype=np.uint64), np.asarray(mults, dtype=np.int64))


def straddling_mults(s, boundaries, run=3):
    """multiplicities of a sorted list of s values in which a run of `run` equal values lies across every position of `boundaries`
    (a run starts one position in front of the boundary), single values elsewhere"""
    mults, pos = [], 0
    bset = sorted(b for b in set(boundaries) if 1 <= b < s)
    while pos < s:
        nxt = next((b for b in bset if b > pos), None)
        if nxt is not None and nxt - 1 == pos and pos + run <= s:
            mults.append(run); pos += run
        else:
            mults.append(1); pos += 1
    return mults


def planted_pairs(s):
    """[(name, A, B, intersect)]: pairs of lists of s values with the intersection worked out by hand; every list is shuffled"""
    rng = np.random.default_rng(1000 + s)
    c = tile_constants()
    w = c["BK_W"]
    base = np.sort(rng.choice(np.arange(1, 64 * s + 64, dtype=np.uint64), size=s + 1, replace=False))     # s + 1 distinct values
    A = base[:s]
    out = [("identical", A, A.copy(), s),
           ("disjoint", A, A + np.uint64(1 << 40), 0),
           ("shifted by one rank", A, base[1:], s - 1),
           ("all equal", np.full(s, 7, dtype=np.uint64), np.full(s, 7, dtype=np.uint64), s),
           ("all equal against one of them", np.full(s, 7, dtype=np.uint64), cat([7], A[:s - 1] + np.uint64(100)), 1),
           ("2^60 against 2^60 + 1", cat([1 << 60], A[:s - 1]),
            cat([(1 << 60) + 1], A[:s - 1]), s - 1),
           ("MaxUint64 and 0", cat([U64_MAX], A[:s - 1]),
            cat([U64_MAX], np.zeros(s - 1)), 1),
           ("0 against MaxUint64", np.zeros(s, dtype=np.uint64), np.full(s, U64_MAX, dtype=np.uint64), 0)]
    if s >= 2:
        out.append(("MaxUint64 and 0, both shared", cat([U64_MAX, 0], A[:s - 2]),
                    cat([0, U64_MAX], A[:s - 2] + np.uint64(1 << 40)), 2))
    if s >= 5:
        out.append(("3 x against 2 x", cat([9, 9, 9], A[:s - 3] + np.uint64(100)),
                    cat([9, 9], A[:s - 2] + np.uint64(1 << 40)), 2))
    # runs of duplicates across the code's boundaries, in sorted positions: the windows of BK_W entries, the positions the threads of
    # the preparation split a sketch at (E = ceil(s / PREP_THREADS) apiece), and — in run-length entries — every BK_W-th distinct value
    e = -(-s // c["PREP_THREADS"])
    for name, bounds, run in (("runs across every window of BK_W positions", range(w, s, w), 3),
                              ("runs across the preparation's thread boundaries", range(e, s, e), 2)):
        mults = straddling_mults(s, bounds, run)
        vals = base[:len(mults)]
        other_m = [max(1, m - 1) for m in mults]                    # the other list holds each run one shorter, and pads with foreign values
        pad = s - sum(other_m)
        B = cat(from_runs(vals, other_m), np.arange(pad, dtype=np.uint64) + np.uint64(1 << 41))
        out.append((name, from_runs(vals, mults), B, sum(other_m)))
    # ... and run-length entries BK_W - 1 and BK_W of every window doubled
    d = max(1, (2 * s) // 3)
    mults = [2 if (k % w in (w - 1, 0) and k > 0) else 1 for k in range(d)]
    while sum(mults) > s:
        mults.pop()
    mults[-1] += s - sum(mults)
    vals = base[:len(mults)]
    ones = [1] * len(mults)
    B = cat(from_runs(vals, ones), np.arange(s - len(mults), dtype=np.uint64) + np.uint64(1 << 41))
    out.append(("doubled entries at the window ends of the run-length form", from_runs(vals, mults), B, len(mults)))
    res = []
    for name, a, b, want in out:
        a = np.asarray(a, dtype=np.uint64); b = np.asarray(b, dtype=np.uint64)
        assert len(a) == s and len(b) == s, (name, len(a), len(b), s)
        res.append((name, rng.permutation(a), rng.permutation(b), int(want)))
    return res


def random_set(n, s, seed, spread=3):
    """n lists of s values drawn with replacement from spread * s values: duplicates inside a list and ties between pairs abound"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 2 ** 63, size=max(2, spread * s), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=max(2, spread * s), dtype=np.uint64)
    return pool[rng.integers(0, len(pool), size=(n, s))]


def planted_set(n, s):
    """the planted lists of planted_pairs(s) (as many as fit) in front of a random set, n lists in all"""
    rows = []
    for _, a, b, _ in planted_pairs(s):
        rows += [a, b]
    rows = rows[:n]
    fill = random_set(n - len(rows), s, 77 + s) if n > len(rows) else np.zeros((0, s), dtype=np.uint64)
    return np.vstack([np.array(rows, dtype=np.uint64).reshape(len(rows), s), fill])


NO_TEST = "the inputs are no test: "
# ragged sizes above one position per thread of the preparation: E = ceil(S / PREP_THREADS) is 2, 3, 4, 9 and 16, the last threads own a
# partial range of positions or none, and the sorting network for the next power of two skips a large share of its comparators
RAGGED_SIZES = (257, 513, 1000, 2049, 4095)


def prep_split(s):
    """(E, threads that own a full range of E positions, positions of the partial one behind them, threads that own nothing)"""
    t = tile_constants()["PREP_THREADS"]
    e = -(-s // t)
    return e, s // e, s % e, t - -(-s // e)


def check_ragged_sizes():
    """what the sizes claim: E > 1, a ragged end, and a network in which many comparators have no upper end"""
    seen = set()
    for s in RAGGED_SIZES:
        e, full, part, idle = prep_split(s)
        assert e > 1 and full * e + part == s, (s, e, full, part)
        assert part or idle, NO_TEST + f"S {s}: every thread of the preparation owns a full range"
        seen.add((part > 0, idle > 0))
        p2 = 1 << (s - 1).bit_length()
        assert p2 > s, NO_TEST + f"S {s} is a power of two: the network skips nothing"
    assert {(True, False), (False, True)} <= seen or (True, True) in seen, NO_TEST + "no size with a partial range, or none with idle threads"


@functools.lru_cache(maxsize=None)
def tied_collection(s):
    """130 sketches whose values come from a small range: ties between pairs abound"""
    m = random_set(130, s, 130 + s, spread=2)
    D = matrix(m)
    off = D[~np.eye(len(m), dtype=bool)]
    assert len(np.unique(off)) * 8 < off.size, NO_TEST + "few ties"
    assert ((off > 0) & (off < 1)).mean() > 0.9, NO_TEST + "distances at the ends"
    m.setflags(write=False); D.setflags(write=False)
    return m, D


def closest_pair(D):
    """(a, b), a < b: the pair with the smallest key (distance, a, b) — the first edge of Kruskal's tree, the first merge of every
    linkage, hit 0 of a's self search"""
    n = len(D)
    iu = np.triu_indices(n, 1)
    at = np.lexsort((iu[1], iu[0], D[iu]))[0]
    return int(iu[0][at]), int(iu[1][at])


def density_set(n, s, seed=9):
    """n lists of s values of very different density over one pool of s distinct values, 0 and the largest uint64 among them: list 0 is s
    copies of one value, list 1 the s distinct values, lists 2 and 3 s copies of MaxUint64 and of 0, the others hold a geometric ladder
    of 2 .. s - 1 distinct values with uneven multiplicities.  The tile's windows then advance at very different rates.  Shuffled"""
    assert n >= 8 and s >= 16
    rng = np.random.default_rng(seed + s)
    inner = np.unique(rng.integers(1, 2 ** 63, size=2 * s, dtype=np.uint64) * np.uint64(2) + np.uint64(1))[:s - 2]
    pool = np.sort(cat([0, U64_MAX], rng.permutation(inner)[:s - 2]))
    assert len(pool) == s and len(np.unique(pool)) == s
    rows = [np.full(s, pool[s // 2], dtype=np.uint64), pool.copy(), np.full(s, U64_MAX, dtype=np.uint64), np.zeros(s, dtype=np.uint64)]
    ladder = np.unique(np.rint(np.geomspace(2, s - 1, n - 4)).astype(np.int64))
    for r in range(n - 4):
        d = int(ladder[r % len(ladder)])
        vals = np.sort(rng.choice(pool[1:-1], size=d - (r % 3 != 0) - (r % 2 != 0), replace=False))
        vals = cat([0] if r % 3 else [], vals, [U64_MAX] if r % 2 else [])
        extra = rng.multinomial(s - d, rng.dirichlet(np.full(d, 0.3)))
        rows.append(from_runs(vals, 1 + extra))
    return np.array([rng.permutation(r) for r in rows], dtype=np.uint64)


def check_density_set(n, s):
    m = density_set(n, s)
    assert m.shape == (n, s)
    distinct = np.array([len(np.unique(r)) for r in m])
    assert distinct[0] == 1 and distinct[1] == s and distinct.min() == 1 and distinct.max() == s, NO_TEST + "no list of one value or none of s"
    assert len(set(distinct.tolist())) >= min(n - 4, 12), NO_TEST + f"the densities are {sorted(set(distinct.tolist()))}"
    assert (m == 0).any(axis=1).sum() >= n // 3 and (m == U64_MAX).any(axis=1).sum() >= n // 3, NO_TEST + "0 and MaxUint64 are rare"
    D = matrix(m)
    off = D[~np.eye(n, dtype=bool)]
    assert ((off > 0) & (off < 1)).mean() > 0.6, NO_TEST + "most distances are 0 or 1"
    assert D[0, 1] == 1.0 - 1.0 / s and D[2, 3] == 1.0 and D[1, 2] == 1.0 - 1.0 / s, "the yardstick on the hand-worked pairs"
    return m, D
