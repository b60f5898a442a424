"""The yardstick of tests/test_gpu_dendrogram.py and tests/test_dendrogram_cpu.py (no test lives here).

Yardstick: D = oracle.pyorc.smash_matrix over the set, W = fmin(D, D.T) off the diagonal, Kruskal over the non-NaN pairs i < j
sorted by (W, i, j) — the edges it keeps, in that order, are the dendrogram: index arrays compared as equal, distances as bits.
offer_rounds restates the OFFER form (per sketch the minimum of (W, partner) over the sketches of other components, per component
the minimum of its members' offers by (W, lo, hi), unite, repeat) on the matrix: it must reproduce Kruskal, and the number of its
passes — the empty closing pass of a forest included — is what stats["rounds"] has to be, because every component picks in every
round.  The sets are tests/cluster_inputs.py's; check_* assert, on the yardstick alone, what the inputs are meant to exercise."""
import functools
import math

import numpy as np

import cluster_inputs as ci
from oracle import pyorc

NO_TEST = ci.NO_TEST
METRICS = ("jaccard", "weightedjaccard")
MULTI_ROUND = (("planted_chains", 8, "weightedjaccard"), ("planted_chains", 33, "weightedjaccard"), ("ordered_chain", "random", "jaccard"),
               ("planted_chains", 8, "jaccard"), ("planted_chains", 33, "jaccard"))


def bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def edge_weights(D):
    """W[i, j] = fmin(D[i, j], D[j, i]): NaN only where both directions are; the diagonal NaN (no self edge)"""
    W = np.fmin(D, D.T)
    np.fill_diagonal(W, np.nan)
    return W


def kruskal(D):
    """-> (a uint32[E], b uint32[E], d float64[E]): the minimum spanning forest of W under the total order (W, i, j), in that order"""
    W = edge_weights(np.asarray(D, dtype=np.float64))
    n = len(W)
    i, j = np.triu_indices(n, 1)
    w = W[i, j]
    keep = ~np.isnan(w)
    i, j, w = i[keep], j[keep], w[keep]
    order = np.lexsort((j, i, w))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    a, b, d = [], [], []
    for at in range(0, len(order), 1 << 16):                        # in pieces: a spanning tree is complete long before the last edge
        piece = order[at:at + (1 << 16)]
        for x, y, h in zip(i[piece].tolist(), j[piece].tolist(), w[piece].tolist()):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
                a.append(x); b.append(y); d.append(h)
        if len(a) == n - 1:                                         # every later edge closes a cycle
            break
    return np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32), np.array(d, dtype=np.float64)


def offer_rounds(D):
    """the offer form on the matrix -> (a, b, d, rounds): rounds counts every pass, the empty one that closes a forest included"""
    W = edge_weights(np.asarray(D, dtype=np.float64))
    n = len(W)
    comp = np.arange(n)
    edges, rounds = set(), 0
    while len(set(comp.tolist())) > 1:
        rounds += 1
        M = np.where((comp[:, None] != comp[None, :]) & ~np.isnan(W), W, np.inf)
        best_p = M.argmin(axis=1)                               # the first minimum: the smaller partner at equal W
        best_d = M[np.arange(n), best_p]
        pick = {}
        for s in range(n):
            if best_d[s] == np.inf:                             # (W <= 1: inf is "no offer")
                continue
            p = int(best_p[s])
            key = (float(best_d[s]), min(s, p), max(s, p))
            c = int(comp[s])
            if c not in pick or key < pick[c]:
                pick[c] = key
        if not pick:
            break
        fresh = sorted(set(pick.values()))
        assert not edges & set(fresh)
        edges |= set(fresh)
        roots = {int(c): int(c) for c in set(comp.tolist())}

        def find(x):
            while roots[x] != x:
                x = roots[x]
            return x
        for _, lo, hi in fresh:
            ra, rb = find(int(comp[lo])), find(int(comp[hi]))
            assert ra != rb, "the picks of a round closed a cycle"
            roots[max(ra, rb)] = min(ra, rb)
        comp = np.array([find(int(c)) for c in comp])
    out = sorted(edges)
    return (np.array([e[1] for e in out], dtype=np.uint32), np.array([e[2] for e in out], dtype=np.uint32),
            np.array([e[0] for e in out], dtype=np.float64), rounds)


def round_bound(n):
    return 0 if n <= 1 else math.ceil(math.log2(n)) + 1


def same_edges(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2])))


def cut_labels(n, a, b, d, tau):
    """the components of the edges with d <= tau, labelled by their smallest member (cluster_inputs' union-find)"""
    keep = d <= tau
    return ci.union_find_labels(n, zip(a[keep].tolist(), b[keep].tolist()))


@functools.lru_cache(maxsize=None)
def named_set(kind, arg, metric):
    """-> (mins, weights, D) of a cluster_inputs set under a metric"""
    if kind == "planted_chains":
        mins, weights, D, _ = ci.planted_chains(arg)
        return mins, weights, D[metric]
    if kind == "random_set":
        mins, weights, per_metric = ci.random_set(arg)
        return mins, weights, per_metric[metric][0]
    if kind == "ordered_chain":
        mins, weights, D = ci.ordered_chain(arg)
        assert metric == "jaccard"
        return mins, weights, D
    if kind == "weighted_set":
        mins, weights, D = ci.weighted_set()
        if metric == "jaccard":
            D = pyorc.smash_matrix(mins, weights, "jaccard")
            D.setflags(write=False)
        return mins, weights, D
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def reference(kind, arg, metric, n=None):
    """Kruskal over the first n sketches of a named set (a pair's distance depends on the pair alone) -> (a, b, d), read-only"""
    D = named_set(kind, arg, metric)[2]
    out = kruskal(D if n is None else D[:n, :n])
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_rounds(kind, arg, metric):
    D = named_set(kind, arg, metric)[2]
    a, b, d, rounds = offer_rounds(D)
    assert same_edges((a, b, d), reference(kind, arg, metric)), NO_TEST + "the offer form does not reproduce Kruskal"
    return rounds


def shapes_set(s):
    """the 257 sketches of the shapes test at sketch size s: the random set for S = 1 (a chain needs 2 * T0 slots), else the chains"""
    return ("random_set", 1) if s == 1 else ("planted_chains", s)


@functools.lru_cache(maxsize=None)
def identical_set(n=65, s=8):
    rng = np.random.default_rng(7400)
    mins = np.tile(rng.integers(0, 1 << 50, size=s, dtype=np.uint64), (n, 1))
    weights = np.tile(-rng.gamma(2.0, 1e-3, size=s), (n, 1))
    return mins, weights


@functools.lru_cache(maxsize=None)
def disjoint_set(n=65, s=8):
    rng = np.random.default_rng(7401)
    mins = (np.arange(n * s, dtype=np.uint64) + np.uint64(1 << 40)).reshape(n, s)
    weights = -rng.gamma(2.0, 1e-3, size=(n, s))
    return mins, weights


def zero_weight_set(n=3, s=8):
    rng = np.random.default_rng(7402)
    return rng.integers(0, 1 << 50, size=(n, s), dtype=np.uint64), np.zeros((n, s))


def check_multi_round():
    """the sets named for multi-round coverage need at least 4 rounds of the offer form"""
    out = {}
    for kind, arg, metric in MULTI_ROUND:
        r = reference_rounds(kind, arg, metric)
        assert r >= 4, NO_TEST + f"{kind}({arg}) {metric}: {r} rounds"
        assert r <= round_bound(257)
        out[(kind, arg, metric)] = r
    return out


def check_weighted_facts():
    """weighted_set's tree holds (X0, X1) at D[X0, X1], not D[X1, X0]; Z hangs on (Y, Z) at 0 alone; (U, V) is at D[V, U] although
    D[U, V] is NaN; the identical pair is at 0"""
    mins, weights, D = ci.weighted_set()
    ci.check_weighted_set()
    a, b, d = reference("weighted_set", None, "weightedjaccard")
    at = {(int(x), int(y)): float(h) for x, y, h in zip(a, b, d)}
    assert len(a) == 64, NO_TEST + "the weighted set is not one tree"
    assert at[(ci.X0, ci.X1)] == D[ci.X0, ci.X1] < 0.5 < D[ci.X1, ci.X0], NO_TEST + "(X0, X1)"
    z = [e for e in at if ci.Z in e]
    assert z == [(ci.Y, ci.Z)] and at[(ci.Y, ci.Z)] == 0 and np.isnan(D[ci.Z, ci.Y]), NO_TEST + "Z is not attached through (Y, Z) alone"
    assert np.isnan(D[ci.U, ci.V]) and at[(ci.U, ci.V)] == D[ci.V, ci.U], NO_TEST + "(U, V)"
    assert at[(ci.I0, ci.I1)] == 0, NO_TEST + "the identical pair"
    return at


def check_ties():
    """every jaccard set has tied heights among its tree's edges"""
    for kind, arg in (("planted_chains", 8), ("planted_chains", 33), ("planted_chains", 512), ("random_set", 1), ("random_set", 8),
                      ("random_set", 33), ("ordered_chain", "ascending"), ("ordered_chain", "descending"), ("ordered_chain", "random"),
                      ("weighted_set", None)):
        d = reference(kind, arg, "jaccard")[2]
        assert len(np.unique(d)) < len(d), NO_TEST + f"{kind}({arg}): no tied heights"
