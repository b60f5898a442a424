"""The yardstick of tests/test_gpu_linkage.py and tests/test_linkage_cpu.py (no test lives here).

Yardstick: D = oracle.pyorc.smash_matrix over the set, W = fmin(D, D.T) off the diagonal, +inf where both directions are NaN and on
the diagonal; then the primitive agglomeration, restated literally: every step takes the argmin of the key (d(p, q), p, q) over the
whole matrix of live pairs p < q — no cache of any kind —, records (p, q, d, size), and rewrites d(p, k) for every other live k by
the method's rule.  Index arrays are compared as equal, distances as bits.  The sets are tests/cluster_inputs.py's and
tests/dendrogram_inputs.py's; check_* assert, on the yardstick alone, what the inputs are meant to exercise."""
import functools

import numpy as np

import cluster_inputs as ci
import dendrogram_inputs as di
from oracle import pyorc

NO_TEST = ci.NO_TEST
METRICS = di.METRICS
METHODS = ("single", "complete", "average")
GRID_N = 1100                                                   # above one workgroup's 1,024 lanes
bits = di.bits


def weights_matrix(D):
    """W[i, j] = fmin(D[i, j], D[j, i]); +inf where both directions are NaN and on the diagonal"""
    D = np.asarray(D, dtype=np.float64)
    W = np.fmin(D, D.T)
    W[np.isnan(W)] = np.inf
    np.fill_diagonal(W, np.inf)
    return W


def agglomerate(D, method):
    """-> (a uint32[M], b uint32[M], d float64[M], size uint32[M]): the merges of the primitive algorithm in the order performed"""
    assert method in METHODS
    W = weights_matrix(D)
    n = len(W)
    U = np.where(np.triu(np.ones((n, n), dtype=bool), 1), W, np.inf)    # the live pairs p < q; everything else +inf
    size = np.ones(n, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    a, b, d, s = [], [], [], []
    while True:
        at = int(U.argmin())                                    # the first minimum in row-major order: the smallest (p, q) at equal d
        p, q = divmod(at, n)
        h = U[p, q]
        if not h < np.inf:
            break
        assert p < q and live[p] and live[q]
        a.append(p); b.append(q); d.append(h); s.append(int(size[p] + size[q]))
        x = np.concatenate([U[:p, p], [np.inf], U[p, p + 1:]])          # d(p, k) for every k
        y = np.concatenate([U[:q, q], [np.inf], U[q, q + 1:]])          # d(q, k)
        if method == "single":
            z = np.minimum(x, y)
        elif method == "complete":
            z = np.maximum(x, y)
        else:
            np_, nq_ = np.float64(size[p]), np.float64(size[q])
            z = ((np_ * x) + (nq_ * y)) / (np_ + nq_)                   # four operations, each rounded on its own; +inf propagates
        live[q] = False
        z[~live] = np.inf
        z[p] = np.inf
        U[:p, p] = z[:p]; U[p, p + 1:] = z[p + 1:]
        U[q, :] = np.inf; U[:, q] = np.inf
        size[p] += size[q]
    return (np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32), np.array(d, dtype=np.float64), np.array(s, dtype=np.uint32))


def same_merges(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2]))
            and np.array_equal(got[3], want[3]))


def finite_components(D):
    W = weights_matrix(D)
    i, j = np.nonzero(np.triu(np.isfinite(W), 1))
    labels = ci.union_find_labels(len(W), zip(i.tolist(), j.tolist()))
    return int((labels == np.arange(len(W))).sum())


def member_sets(n, a, b):
    """the members of the cluster every merge creates, in merge order"""
    members = {i: frozenset([i]) for i in range(n)}
    name = list(range(n))                                       # member -> the name of its cluster is found through the sets

    def find(x):
        while name[x] != x:
            x = name[x]
        return x
    out = []
    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        rx, ry = find(x), find(y)
        assert rx != ry
        lo, hi = min(rx, ry), max(rx, ry)
        members[lo] = members[lo] | members.pop(hi)
        name[hi] = lo
        out.append(members[lo])
    return out


@functools.lru_cache(maxsize=None)
def grid_set():
    """GRID_N sketches of 8 slots over a shared base, and D per metric"""
    n, s = GRID_N, 8
    rng = np.random.default_rng(7500)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    mins = np.empty((n, s), dtype=np.uint64)
    for i in range(n):
        keep = rng.random(s) < (0.2 + 0.6 * rng.random())
        mins[i] = np.where(keep, base, rng.integers(0, 194481, size=s).astype(np.uint64))
    weights = -rng.gamma(2.0, 1e-3, size=(n, s))
    weights[rng.random((n, s)) < 0.05] *= -1
    D = {m: pyorc.smash_matrix(mins, weights, m) for m in METRICS}
    for x in (mins, weights, *D.values()):
        x.setflags(write=False)
    return mins, weights, D


@functools.lru_cache(maxsize=None)
def named_set(kind, arg, metric):
    """-> (mins, weights, D): dendrogram_inputs' named sets, "grid_set", "identical_set", "disjoint_set" and "zero_weight_set" """
    if kind == "grid_set":
        mins, weights, D = grid_set()
        return mins, weights, D[metric]
    if kind in ("identical_set", "disjoint_set", "zero_weight_set"):
        mins, weights = getattr(di, kind)()
        D = pyorc.smash_matrix(mins, weights, metric)
        D.setflags(write=False)
        return mins, weights, D
    return di.named_set(kind, arg, metric)


@functools.lru_cache(maxsize=None)
def reference(kind, arg, metric, method, n=None):
    """the yardstick over the first n sketches of a named set (a pair's distance depends on the pair alone), read-only"""
    D = named_set(kind, arg, metric)[2]
    out = agglomerate(D if n is None else D[:n, :n], method)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tie_free_set(n=64, s=64):
    """a random weightedjaccard set whose symmetric input has no two equal entries (for the comparison with SciPy).  A subject's
    distance depends on WHICH of its slots the other sketch shares: 64 slots kept with probability 1 / 2 give every pair its own"""
    rng = np.random.default_rng(7600)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    mins = np.empty((n, s), dtype=np.uint64)
    for i in range(n):
        mins[i] = np.where(rng.random(s) < 0.5, base, rng.integers(1 << 40, 1 << 50, size=s).astype(np.uint64))
    weights = -rng.gamma(2.0, 1e-3, size=(n, s))
    D = pyorc.smash_matrix(mins, weights, "weightedjaccard")
    W = weights_matrix(D)
    off = W[np.triu_indices(n, 1)]
    assert np.isfinite(off).all() and len(np.unique(off)) == len(off), NO_TEST + "the tie-free set has ties"
    return mins, weights, D


JACCARD_SETS = (("planted_chains", 8), ("planted_chains", 33), ("random_set", 1), ("random_set", 8), ("random_set", 33), ("grid_set", None),
                ("weighted_set", None))


def check_ties():
    """every jaccard set has tied heights, under every method"""
    for kind, arg in JACCARD_SETS:
        for method in METHODS:
            if kind == "grid_set" and method != "complete":
                continue                                        # (one pass of the large set is enough here)
            d = reference(kind, arg, "jaccard", method)[2]
            assert len(np.unique(d)) < len(d), NO_TEST + f"{kind}({arg}) {method}: no tied heights"


def check_complete_differs_from_single():
    """the planted chains: at the chains' own threshold single linkage holds a chain together, complete linkage does not"""
    n, tau = 257, ci.chain_tau(8)
    s_ = reference("planted_chains", 8, "jaccard", "single")
    c_ = reference("planted_chains", 8, "jaccard", "complete")
    ls, lc = di.cut_labels(n, s_[0], s_[1], s_[2], tau), di.cut_labels(n, c_[0], c_[1], c_[2], tau)
    assert not np.array_equal(ls, lc), NO_TEST + "complete and single linkage give the same partition at the chains' threshold"
    assert np.array_equal(ls, ci.components(named_set("planted_chains", 8, "jaccard")[2], tau)[0])
    assert (lc == np.arange(n)).sum() > (ls == np.arange(n)).sum(), NO_TEST + "complete linkage does not split the chains"
    return tau


Z2 = 20                                                         # weighted_forest_set: a second sketch with an all-zero weight row


@functools.lru_cache(maxsize=None)
def weighted_forest_set():
    """cluster_inputs.weighted_set — directional distances (X0, X1), a one-direction NaN (U, V), an all-zero subject Z — has no pair
    that is NaN in BOTH directions: every other sketch reaches Z through its own row.  Here Z2 gets an all-zero weight row too, so
    that (Z, Z2) is NaN both ways: W = +inf, and no cluster that holds Z ever merges with one that holds Z2 under complete or
    average linkage, although the finite graph is connected"""
    mins, weights, _ = ci.weighted_set()
    weights = weights.copy()
    weights[Z2] = 0.0
    D = pyorc.smash_matrix(mins, weights, "weightedjaccard")
    for x in (weights, D):
        x.setflags(write=False)
    return mins, weights, D


def check_weighted_forest():
    """(Z, Z2) is the double-NaN pair: single linkage still gives one tree (n - 1 merges = n - the components of the finite graph),
    complete and average linkage leave more than one cluster"""
    mins, weights, D = weighted_forest_set()
    ci.check_weighted_set()
    assert np.isnan(D[ci.Z, Z2]) and np.isnan(D[Z2, ci.Z]), NO_TEST + "no double-NaN pair"
    assert D[ci.X0, ci.X1] != D[ci.X1, ci.X0] and np.isnan(D[ci.U, ci.V]) and not np.isnan(D[ci.V, ci.U]), NO_TEST + "directions"
    out = {}
    for method in METHODS:
        a, b, d, s = agglomerate(D, method)
        out[method] = len(D) - len(a)
        pairs = [m for m in member_sets(len(D), a, b) if ci.Z in m and Z2 in m]
        assert method == "single" or not pairs, NO_TEST + "Z and Z2 share a cluster"
    assert out["complete"] > 1 and out["average"] > 1, NO_TEST + f"one cluster everywhere: {out}"
    assert out["single"] == finite_components(D) == 1, NO_TEST + "single linkage leaves the components of the finite graph"
    return out


def check_stars():
    """identical sketches: every height 0, the order is the key's alone — (0, 1), (0, 2), ...; disjoint ones: every height 1"""
    for kind, h in (("identical_set", 0.0), ("disjoint_set", 1.0)):
        for metric in METRICS:
            for method in METHODS:
                a, b, d, s = reference(kind, None, metric, method)
                assert not a.any() and b.tolist() == list(range(1, 65)) and (d == h).all() and s.tolist() == list(range(2, 66)), \
                    NO_TEST + f"{kind} {metric} {method}: not a star at sketch 0"
    for method in METHODS:
        assert len(reference("zero_weight_set", None, "weightedjaccard", method)[0]) == 0, NO_TEST + "all-zero weights merge"
