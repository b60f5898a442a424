"""The yardstick, inputs and check_* functions of tests/test_gpu_linkage_scale.py and tests/test_linkage_scale_cpu.py (no test lives
here): hulk_linkage past one chunk of LINK_CHUNK merges, and on forests that end at the chunk's border.

Yardstick: linkage_inputs.agglomerate takes a literal argmin over the whole matrix every step — O(N^3), about a minute at N = 4161.
agglomerate_cached restates the same algorithm with a per-row cache of the nearest live j > i under the key (bits, j): a row is
rescanned when its cached column was p or q, and so is row p; every other row compares the one entry of it that changed.  That is
hulk_linkage.hip's own idea, so it is no yardstick until tests/test_linkage_scale_cpu.py has held it to the literal one on every set
the small suite uses and on the first 600 sketches of every set here.  Plain numpy, float64; the average rule stays four separately
rounded operations.

Every case is a prefix D[:n, :n] of the one matrix of its set (a pair's distance depends on the pair alone); every n is derived from
LINK_CHUNK, which is read out of hulk_linkage.hip.  With C = LINK_CHUNK:
  dense    4161 sketches over a shared base whose slot 0 everybody keeps: every pair is below 1.0, so the last merges of a full tree
           are no tail of merges at exactly 1.0 (scale_inputs.chains has 66 components below 1.0: its last 65 merges under every
           method are at 1.0, all 64 of chunk two among them).  Full trees with N - 1 = C - 1, C, C + 1 and at N = 4161
  chains   scale_inputs.chains at its whole N: ties everywhere and the tail at 1.0 (jaccard, weighted jaccard; bottomk from
           scale_inputs.give_matrix)
  far_pairs  scale_inputs.far_pairs at its whole N: its twins (4097, 4160) and (4130, 4131) are pairs at 0 whose smaller member lies
           behind row 4 * 1,024 — the row k_linkage_pick's strided loop reads in its fifth trip has to win the pick
  border   chains with all-zero weight rows at ZERO_BORDER: those sketches are NaN both ways from each other (W = +inf), every other
           sketch reaches them through its own row; complete and average linkage stop with m clusters after n - m merges.  The
           prefixes C + 5, C + 7 and C + 9 hold 6, 7 and 8 of them, the last one on the prefix's highest index: C - 1, C and C + 1
           merges — "finished" is raised by the pick in the last slot of chunk one, in the first slot of chunk two and in the second
  inside   chains with every weight row zero but KEPT of them: KEPT merges at N = 4161, and 3 * (C - KEPT) queued launches that
           return at once; single linkage on it is one tree of N - 1 merges"""
import functools
import os
import re

import numpy as np

import linkage_inputs as li
import scale_inputs as sc
from conftest import ROOT
from oracle import pyorc

NO_TEST = li.NO_TEST
METHODS = li.METHODS
bits = li.bits
N, S = sc.N, sc.S
KEPT = 300                                                      # inside: the sketches that keep their weights
PREFIX = 600                                                    # the two yardsticks are compared on the first PREFIX sketches of a set


def link_chunk():
    """LINK_CHUNK as hulk_linkage.hip states it"""
    text = open(os.path.join(ROOT, "hulk_amd", "csrc", "hulk_linkage.hip")).read()
    found = re.findall(r"^constexpr uint32_t LINK_CHUNK = (\d+);", text, re.M)
    assert len(found) == 1, "hulk_linkage.hip no longer states `constexpr uint32_t LINK_CHUNK = <number>;`: the sizes here are derived from it"
    c = int(found[0])
    assert 1024 < c and c + 9 <= N, (f"LINK_CHUNK = {c}: the sets here have {N} sketches and need LINK_CHUNK + 9 of them (and more than "
                                     "k_linkage_pick's 1,024 lanes): with this value the tests would run one chunk only — resize the sets")
    return c


C = link_chunk()
FULL_NS = (C, C + 1, C + 2, N)                                  # N - 1 = C - 1, C, C + 1; and 64 merges in chunk two
BORDER = {C - 1: (C + 5, 6), C: (C + 7, 7), C + 1: (C + 9, 8)}  # merges -> (prefix, zeroed sketches in it)
ZERO_BORDER = (3, 300, 700, 2048, 3500, C + 4, C + 6, C + 8)   # low, middle, and the highest index of each prefix


# ---- the cached yardstick ----------------------------------------------------------------------------------------------------------
def agglomerate_cached(D, method, stats=None):
    """linkage_inputs.agglomerate's outputs, from a cache (nnd[i], nn[i]) = min over live j > i of (W[i, j], j) per row.  W >= 0 or
    +inf, no NaN: a double orders like its bits.  stats["rows_rescanned"]: the rows scanned, the first fill's n included"""
    assert method in METHODS
    W = li.weights_matrix(D)                                    # (a copy: symmetric, +inf on the diagonal)
    n = len(W)
    live = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.int64)
    nnd = np.full(n, np.inf)
    nn = np.full(n, -1, dtype=np.int64)

    def rescan(i):
        row = np.where(live[i + 1:], W[i, i + 1:], np.inf)
        j = int(row.argmin()) if len(row) else 0                # the first minimum: the smallest j at equal distance
        if len(row) and row[j] < np.inf:
            nnd[i], nn[i] = row[j], i + 1 + j
        else:
            nnd[i], nn[i] = np.inf, -1

    if n > 1:
        U = np.where(np.triu(np.ones((n, n), dtype=bool), 1), W, np.inf)
        first = U.argmin(axis=1)
        found = U[np.arange(n), first] < np.inf
        nnd[found], nn[found] = U[np.arange(n), first][found], first[found]
        del U
    a, b, d, s = [], [], [], []
    scanned = n if n > 1 else 0
    while True:
        p = int(nnd.argmin())                                   # the first minimum: the smallest p at equal distance
        h = nnd[p]
        if not h < np.inf:
            break
        q = int(nn[p])
        assert p < q and live[p] and live[q]
        a.append(p); b.append(q); d.append(h); s.append(int(size[p] + size[q]))
        x, y = W[p], W[q]
        if method == "single":
            z = np.minimum(x, y)
        elif method == "complete":
            z = np.maximum(x, y)
        else:
            np_, nq_ = np.float64(size[p]), np.float64(size[q])
            z = ((np_ * x) + (nq_ * y)) / (np_ + nq_)           # four operations, each rounded on its own; +inf propagates
        live[q] = False
        size[p] += size[q]
        z[~live] = np.inf
        z[p] = np.inf
        W[p, :] = z
        W[:, p] = z
        nnd[q], nn[q] = np.inf, -1
        stale = live & ((nn == p) | (nn == q))                  # (nn[k] is above k: these rows are below q)
        stale[p] = True
        zk, old, c = z[:p], nnd[:p], nn[:p]
        take = live[:p] & ~stale[:p] & (zk < np.inf) & ((zk < old) | ((zk == old) & (p < c)))
        nnd[:p][take] = zk[take]
        nn[:p][take] = p
        for i in np.nonzero(stale)[0].tolist():
            rescan(i)
        scanned += int(stale.sum())
    if stats is not None:
        stats["rows_rescanned"] = scanned
    return (np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32), np.array(d, dtype=np.float64), np.array(s, dtype=np.uint32))


# ---- the sets ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense():
    """-> (mins, weights, {metric: D}): every sketch is a shared base with slot 0 kept and every other slot kept with a probability
    of its own between 0.3 and 0.9; the weights as everywhere, a twentieth of them positive"""
    rng = np.random.default_rng(9500)
    base = rng.integers(0, 1 << 50, size=S, dtype=np.uint64)
    keep = rng.random((N, S)) < (0.3 + 0.6 * rng.random((N, 1)))
    keep[:, 0] = True
    mins = np.where(keep, base, rng.integers(0, 1 << 50, size=(N, S), dtype=np.uint64))
    weights = -rng.gamma(2.0, 1e-3, size=(N, S))
    weights[rng.random((N, S)) < 0.05] *= -1
    D = sc.matrices(mins, weights)
    sc.frozen(mins, weights, *D.values())
    return mins, weights, D


def zeroed(kind):
    if kind == "border":
        return np.array(ZERO_BORDER)
    rng = np.random.default_rng(9600)
    kept = np.sort(rng.permutation(np.arange(1, N - 1))[:KEPT])  # (sketch 0 and the highest, N - 1, are zeroed)
    return np.setdiff1d(np.arange(N), kept)


@functools.lru_cache(maxsize=None)
def forest_set(kind):
    """scale_inputs.chains with the weight rows of zeroed(kind) all zero -> (mins, weights, D under weightedjaccard)"""
    mins, weights = sc.chains()[:2]
    weights = weights.copy()
    weights[zeroed(kind)] = 0.0
    D = pyorc.smash_matrix(mins, weights, "weightedjaccard")
    sc.frozen(weights, D)
    return mins, weights, D


def arrays(name):
    """-> (mins, weights) of a set"""
    if name == "dense":
        return dense()[:2]
    if name in sc.SETS:
        return sc.SETS[name]()[:2]
    return forest_set(name)[:2]


def matrix(name, metric):
    if name == "dense":
        return dense()[2][metric] if metric in sc.ORACLE_METRICS else sc.matrix(name, metric)
    if name in sc.SETS:
        return sc.matrix(name, metric)
    assert metric == "weightedjaccard"
    return forest_set(name)[2]


# ---- the cases: (set, metric, method, n) -------------------------------------------------------------------------------------------
FOREST_CASES = ([("border", "weightedjaccard", method, BORDER[m][0]) for m in sorted(BORDER) for method in ("complete", "average")]
                + [("inside", "weightedjaccard", method, N) for method in ("complete", "average", "single")])
FULL_BORDER_CASES = [("dense", metric, method, n) for n in FULL_NS[:3] for metric in sc.ORACLE_METRICS for method in METHODS]
WHOLE_CASES = ([(name, metric, method, N) for name in ("dense", "chains") for metric in sc.ORACLE_METRICS for method in ("complete", "average")]
               + [(name, metric, "single", N) for name in ("dense", "chains") for metric in sc.ORACLE_METRICS]
               + [("far_pairs", metric, method, N) for metric in sc.ORACLE_METRICS for method in ("complete", "average")])
BOTTOMK_CASES = [("dense", "bottomk", "complete", n) for n in FULL_NS] + [("chains", "bottomk", "complete", N)]
ORACLE_CASES = FOREST_CASES + FULL_BORDER_CASES + WHOLE_CASES      # (the order in which cases would be dropped from the end)


def case_id(case):
    return "-".join(str(x) for x in case)


@functools.lru_cache(maxsize=None)
def reference(name, metric, method, n):
    """the cached yardstick over the first n sketches of a set, read-only"""
    st = {}
    out = sc.frozen(*agglomerate_cached(matrix(name, metric)[:n, :n], method, st))
    _rescans[(name, metric, method, n)] = st["rows_rescanned"]
    return out


_rescans = {}


def rows_rescanned(case):
    """the rows the yardstick scanned: the rule that picks them is hulk_linkage.hip's (the module's docstring), so is the number"""
    reference(*case)
    return _rescans[tuple(case)]


def wanted_merges(case):
    """the number of merges a case is built to have"""
    name, metric, method, n = case
    if name == "border" and method != "single":
        return n - int((zeroed("border") < n).sum())
    if name == "inside" and method != "single":
        return KEPT
    return n - 1


# ---- the checks ("the inputs are no test") -----------------------------------------------------------------------------------------
def check_sizes():
    """the Ns follow LINK_CHUNK: a full tree that ends inside chunk one, at its end and one merge behind it; forests of C - 1, C and
    C + 1 merges whose highest sketch is zeroed; k_linkage_pick's loop in its fifth trip; k_linkage_sym's last tile one column wide"""
    assert [n - 1 for n in FULL_NS[:3]] == [C - 1, C, C + 1] and FULL_NS[3] == N > C + 2
    assert (N - 1) // 1024 == 4, NO_TEST + "k_linkage_pick's strided loop does not reach its fifth trip"
    assert (N + 31) // 32 == 131 and N % 32 == 1, NO_TEST + "k_linkage_sym's last tile is not one column wide"
    assert (N + 15) // 16 == 261, NO_TEST + "rows_rescanned is not summed over 261 groups"
    z = zeroed("border")
    for merges, (n, m) in BORDER.items():
        assert C < n <= N and int((z < n).sum()) == m and n - m == merges and n - 1 in z, NO_TEST + f"border {merges}"
    assert z.min() < 32 and any(1024 < i < C - 1024 for i in z.tolist())
    zi = zeroed("inside")
    assert len(zi) == N - KEPT and zi[0] == 0 and zi[-1] == N - 1 and 100 <= KEPT <= 999 and N > C
    for kind in ("border", "inside"):
        weights = forest_set(kind)[1]
        rows = np.nonzero(~weights.any(axis=1))[0]
        assert np.array_equal(rows, zeroed(kind)), NO_TEST + f"{kind}: the all-zero weight rows"


def check_merge_counts(case):
    """the yardstick's merge count is exactly the one the case is built for"""
    got = len(reference(*case)[0])
    assert got == wanted_merges(case), NO_TEST + f"{case_id(case)}: the yardstick has {got} merges, the case is built for {wanted_merges(case)}"
    return got


def check_ties(case):
    """a jaccard (or bottomk) case has tied heights"""
    d = reference(*case)[2]
    assert len(np.unique(d)) < len(d), NO_TEST + f"{case_id(case)}: no tied heights"


def check_late_merges(case):
    """a full tree past the chunk: at least one merge of chunk two is below 1.0 -> how many are"""
    name, metric, method, n = case
    d = reference(*case)[2]
    assert len(d) == n - 1 > C
    late = int((d[C:] < 1.0).sum())
    assert late >= 1, NO_TEST + f"{case_id(case)}: the {len(d) - C} merges of chunk two are all at 1.0 or above"
    return late


PICK_THREADS = 1024                                             # LINK_PICK_THREADS: a trip of k_linkage_pick's loop


def check_fifth_trip(case):
    """some merge's p lies in the rows k_linkage_pick reads in its fifth trip, and it is not the last word: a later merge has a
    smaller p (losing the trip changes the order, not only the end) -> those merges"""
    a = reference(*case)[0]
    late = np.nonzero(a >= 4 * PICK_THREADS)[0]
    assert len(late) and (a[late[0]:] < 4 * PICK_THREADS).any(), NO_TEST + f"{case_id(case)}: no merge is picked from a row of the fifth trip"
    return len(late)


def check_average_steps_down(case):
    """average linkage: a height below its predecessor -> (how many, a message that says so when there is none)"""
    d = reference(*case)[2]
    down = int((np.diff(d) < 0).sum())
    return down, (f"{case_id(case)}: {down} heights step down" if down else
                  f"{case_id(case)}: NO height steps down in this set — the average rule's heights are ascending here")


def check_forest(case):
    """complete and average linkage on a forest set: exactly m clusters are left and none holds two zeroed sketches"""
    name, metric, method, n = case
    a, b, d, s = reference(*case)
    z = zeroed(name)
    z = z[z < n]
    label = np.arange(n)
    for x, y in zip(a.tolist(), b.tolist()):                    # (b is a cluster's name when it merges: its label is itself)
        assert label[x] == x and label[y] == y
        label[label == y] = x
    assert n - len(a) == len(z) == len(np.unique(label)), NO_TEST + f"{case_id(case)}: {n - len(a)} clusters left, {len(z)} zeroed sketches"
    assert len(np.unique(label[z])) == len(z), NO_TEST + f"{case_id(case)}: two zeroed sketches share a cluster"
    D = matrix(name, metric)[:n, :n]
    W = li.weights_matrix(matrix(name, metric)[:n, :n])
    rest = np.setdiff1d(np.arange(n), z)
    assert np.isinf(W[np.ix_(z, z)]).all(), NO_TEST + f"{case_id(case)}: two zeroed sketches at a finite distance"
    assert len(rest) and (np.isfinite(W[rest]).sum(axis=1) == n - 1).all(), NO_TEST + f"{case_id(case)}: the finite graph is not connected through every other sketch"
    return len(z)


def check_case(case):
    """every condition a case has to meet, on the yardstick alone -> facts to print"""
    name, metric, method, n = case
    facts = {"merges": check_merge_counts(case)}
    if metric != "weightedjaccard":
        check_ties(case)
    if name == "dense":
        if n - 1 > C:
            facts["chunk two below 1.0"] = check_late_merges(case)
    if name in ("border", "inside") and method != "single":
        facts["clusters"] = check_forest(case)
    if name == "far_pairs":
        facts["picked in the fifth trip"] = check_fifth_trip(case)
    if method == "average":
        facts["steps down"] = check_average_steps_down(case)[1]
    return facts


# ---- the three identities that need no yardstick of the merge order ------------------------------------------------------------------
U53 = np.longdouble(2.0) ** -53


def cluster_pair_facts(D, a, b):
    """per merge t, from D and the merges alone: (min, max and — in np.longdouble — the mean of W[A x B] over the two clusters it
    joins, the depth of the merge in the tree: 1 + the larger depth of the two; a sketch has depth 0).  Every pair lies across exactly
    one merge: O(N^2) in total"""
    W = li.weights_matrix(D)
    n = len(W)
    members = {i: np.array([i]) for i in range(n)}
    depth = np.zeros(n, dtype=np.int64)
    lo, hi, mean, dep = [], [], [], []
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        A, B = members[x], members.pop(y)
        block = W[np.ix_(A, B)]
        lo.append(block.min()); hi.append(block.max())
        mean.append(block.astype(np.longdouble).sum() / np.longdouble(block.size))
        depth[x] = 1 + max(depth[x], depth[y])
        dep.append(int(depth[x]))
        members[x] = np.concatenate([A, B])
    return np.array(lo), np.array(hi), np.array(mean, dtype=np.longdouble), np.array(dep, dtype=np.int64)


def assert_cluster_pair_identity(D, method, merges, what):
    """single: a height's bits are min W[A x B]; complete: max W[A x B]; average: every finite height h is within
    ((1 + 2^-53)^(3 * depth) - 1) relative of the mean of W[A x B].  The bound: a level of the update is two products, a sum and a
    quotient of terms >= 0 with exact sizes — the two products round side by side, so three roundings of at most 2^-53 each lie on
    any path — and `depth` is the depth of that merge in the returned tree.  (d(A, B) is updated when A grows and when B grows, so a
    path from a height down to an entry of W can hold depth(A) + depth(B) levels, up to 2 * (depth - 1): the bound is the tighter
    one of the two on purpose, and independent roundings use a quarter of it at most on the sets here.  The long-double mean's own
    error, about 20 * 2^-64, is three orders below the bound of the first level at which a rounding can occur.)
    -> the largest |h - mean| / (bound * mean) seen"""
    a, b, d, size = merges
    lo, hi, mean, depth = cluster_pair_facts(D, a, b)
    if method == "single":
        bad = np.nonzero(bits(d) != bits(lo))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} heights are not the smallest distance between the two clusters, first at merge {bad[:3].tolist()}"
        return 0.0
    if method == "complete":
        bad = np.nonzero(bits(d) != bits(hi))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} heights are not the largest distance between the two clusters, first at merge {bad[:3].tolist()}"
        return 0.0
    assert np.isfinite(d).all() and np.isfinite(mean.astype(np.float64)).all(), f"{what}: a merge at +inf"
    bound = (np.longdouble(1.0) + U53) ** (3 * depth).astype(np.longdouble) - np.longdouble(1.0)
    err = np.abs(d.astype(np.longdouble) - mean)
    bad = np.nonzero(err > bound * mean)[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} heights are not the mean distance between the two clusters within 3 roundings a level, first at merge "
                           f"{bad[:3].tolist()}: {[(float(d[i]).hex(), float(mean[i]).hex(), int(depth[i])) for i in bad[:3]]}")
    used = err[mean > 0] / (bound * mean)[mean > 0]
    return float(used.max()) if len(used) else 0.0
