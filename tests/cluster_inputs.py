"""The yardstick and the input generators of tests/test_gpu_cluster.py and tests/test_cluster_cpu.py (no test lives here).

Yardstick: oracle.pyorc.smash_matrix over the set, then a plain Python union-find — edges where (D <= tau) | (D.T <= tau) off the
diagonal, label = the smallest member, links = ((D <= tau) & ~eye).sum().  Every generator comes with a check_* function that
asserts, on the yardstick alone, that its inputs test what they are meant to test ("the inputs are no test" otherwise); the CPU
suite runs these checks without a device, the GPU tests run them again before they compare."""
import functools

import numpy as np

from oracle import pyorc

NO_TEST = "the inputs are no test: "
BANDS = (0, 32, 96)
NS = (1, 2, 31, 32, 33, 63, 64, 65, 257)
T0 = {8: 2, 33: 3, 512: 7}                                  # fresh slots per chain step at each sketch size
# chain neighbours are planted at these index pairs: tile edges of the subjects (32) and the others (64), both directions across
# them, the two ends of the set, and for band_rows 32 / 96 the last row of a band and the first of the next ((31, 32), (63, 64) /
# (95, 96)); (0, N - 1) joins the first band and the last one
BRIDGES = ((31, 32), (32, 95), (63, 64), (64, 33), (0, 256), (95, 96))
PATH_HEAD = (256, 0, 31, 32, 95, 96, 63, 64, 33)            # the first chain runs through these indices in this order
CHAIN_SIZES = (100, 70, 2, 30, 2)                           # > 64 twice, 2 twice; the other 53 sketches are singletons


def union_find_labels(n, edges):
    """plain sequential union-find: label[i] = the smallest member of i's component"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for a, b in edges:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], dtype=np.uint32)


def components(D, tau, rule="or", without=None):
    """-> (labels, links, clusters) of the issue's rule from the matrix D; rule "and": both directions must hold (what the result
    would be if one direction were not enough); without: an unordered pair whose edge is left out (bridge check)"""
    n = len(D)
    le = D <= tau                                           # (False for NaN)
    np.fill_diagonal(le, False)
    adj = (le | le.T) if rule == "or" else (le & le.T)
    if without is not None:
        a, b = without
        adj = adj.copy(); adj[a, b] = adj[b, a] = False
    labels = union_find_labels(n, np.argwhere(np.triu(adj)))
    return labels, int(le.sum()), int((labels == np.arange(n)).sum())


def is_bridge(D, tau, pair):
    a, b = pair
    le = D <= tau
    if a == b or not (le[a, b] or le[b, a]):
        return False
    return components(D, tau, without=pair)[2] == components(D, tau)[2] + 1


def chain(rng, length, s, t0):
    """c0 random; c(t+1) = c(t) with t0 fresh slots in a window that moves on: neighbours differ in exactly t0 slots, sketches two
    or more steps apart in at least 2 * t0 (s >= 2 * t0: consecutive windows do not overlap)"""
    out = np.empty((length, s), dtype=np.uint64)
    out[0] = rng.integers(0, 1 << 50, size=s, dtype=np.uint64)
    for t in range(1, length):
        out[t] = out[t - 1]
        at = (np.arange(t0) + (t - 1) * t0) % s
        out[t, at] = rng.integers(0, 1 << 50, size=t0, dtype=np.uint64)
    return out


def chain_tau(s):
    return 1.0 - ((s - T0[s]) / s)                          # the very double the distance of two chain neighbours is


@functools.lru_cache(maxsize=None)
def planted_chains(s):
    """257 sketches of s slots: five chains (CHAIN_SIZES) and 53 fresh random sketches, placed by a fixed permutation that puts
    chain neighbours at BRIDGES.  -> (mins, weights, {metric: D}, members: the index lists of the chains in chain order)"""
    n, t0 = 257, T0[s]
    rng = np.random.default_rng(7000 + s)
    free = [i for i in rng.permutation(n).tolist() if i not in PATH_HEAD]
    mins = np.empty((n, s), dtype=np.uint64)
    members = []
    for k, size in enumerate(CHAIN_SIZES):
        idx = (list(PATH_HEAD) if k == 0 else []) + [free.pop() for _ in range(size - (len(PATH_HEAD) if k == 0 else 0))]
        mins[idx] = chain(rng, size, s, t0)
        members.append(idx)
    mins[free] = rng.integers(0, 1 << 50, size=(len(free), s), dtype=np.uint64)
    weights = -rng.gamma(2.0, 1e-3, size=(n, s))
    weights[rng.random((n, s)) < 0.05] *= -1
    D = {m: pyorc.smash_matrix(mins, weights, m) for m in ("jaccard", "weightedjaccard")}
    for a in (mins, weights, *D.values()):
        a.setflags(write=False)
    return mins, weights, D, members


def check_planted_chains(s):
    mins, weights, D, members = planted_chains(s)
    J, tau = D["jaccard"], chain_tau(s)
    assert 0 < tau < 1, NO_TEST + "tau"
    labels, links, clusters = components(J, tau)
    for idx in members:
        for a, b in zip(idx, idx[1:]):
            assert J[a, b] == tau and J[b, a] == tau, NO_TEST + "chain neighbours are not at exactly tau"
        assert (labels[idx] == min(idx)).all(), NO_TEST + "a chain is not one component"
    assert links == 2 * sum(len(idx) - 1 for idx in members), NO_TEST + "a link that is not between chain neighbours"
    for pair in BRIDGES:
        assert is_bridge(J, tau, pair), NO_TEST + f"{pair} is no bridge"
    sizes = np.bincount(labels)
    assert (sizes > 1).sum() >= 3 and (sizes == 1).sum() >= 3, NO_TEST + "too few components / singletons"
    assert {1, 2} <= set(sizes.tolist()) and sizes.max() > 64, NO_TEST + "component sizes"
    assert sorted(sizes[sizes > 0].tolist()) == sorted([1] * 53 + list(CHAIN_SIZES)), NO_TEST + "the components are not the chains"
    below = components(J, np.nextafter(tau, 0.0))
    assert below[2] == len(J) and below[1] == 0, NO_TEST + "one ulp below tau something still links"
    return tau, (labels, links, clusters)


def shapes_plan(s):
    """the set and, per metric, (D, tau) of test_planted_shapes: S = 1 the random set at its 10 % quantile; otherwise the planted
    chains — jaccard at the chains' own tau, weightedjaccard at the median of the chain neighbours' weighted distances (about half
    of the chain links hold: the chains fall into pieces).  Asserts that at N = 257 something links and not everything does"""
    if s == 1:
        mins, weights, per_metric = random_set(1)
        check_random_set(1)
        plan = {m: (per_metric[m][0], per_metric[m][1][1]) for m in per_metric}
    else:
        mins, weights, D, members = planted_chains(s)
        tau, _ = check_planted_chains(s)
        W = D["weightedjaccard"]
        near = np.array([W[a, b] for idx in members for a, b in zip(idx, idx[1:])])
        plan = {"jaccard": (D["jaccard"], tau), "weightedjaccard": (W, float(np.quantile(near, 0.5, method="lower")))}
    for metric, (D, tau) in plan.items():
        _, links, clusters = components(D, tau)
        assert 0 < links and 1 < clusters < 257, NO_TEST + f"S {s} {metric}: nothing links, or everything does ({links} links, {clusters} clusters)"
    return mins, weights, plan


@functools.lru_cache(maxsize=None)
def ordered_chain(order):
    """a chain of 257 (S = 33) placed in ascending index order, in descending order, or in a fixed random order"""
    s, n = 33, 257
    rng = np.random.default_rng(7100)
    c = chain(rng, n, s, T0[s])
    place = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "random": np.random.default_rng(7101).permutation(n)}[order]
    mins = np.empty_like(c)
    mins[place] = c
    weights = -rng.gamma(2.0, 1e-3, size=(n, s))
    D = pyorc.smash_matrix(mins, weights, "jaccard")
    for a in (mins, weights, D):
        a.setflags(write=False)
    return mins, weights, D


def check_ordered_chain(order):
    mins, weights, D = ordered_chain(order)
    tau = chain_tau(33)
    labels, links, clusters = components(D, tau)
    assert clusters == 1 and not labels.any() and links == 2 * 256, NO_TEST + "the chain is not one component held by neighbour links"
    assert components(D, np.nextafter(tau, 0.0))[2] == 257, NO_TEST + "one ulp below tau something still links"
    return tau, (labels, links, clusters)


# indices of the planted sketches of weighted_set
X0, X1, Y, Z, U, V, I0, I1 = 31, 32, 5, 64, 40, 41, 10, 50


@functools.lru_cache(maxsize=None)
def weighted_set():
    """65 sketches of 8 slots for weightedjaccard.  X0 / X1 (across the tile edge 31 | 32) share slots 0-3; X0's weight lies on
    them, X1's on the others: d(X0, X1) <= 0.5 < d(X1, X0), and nothing else links either of them to anything — a bridge in one
    direction only.  Z (index 64: the third subject tile, the second tile of others) has an all-zero weight row — NaN as subject —
    and Y's mins: it is linked through Y's row alone.  U carries an Inf weight, on a slot it shares with V.  I0 / I1 are byte-identical."""
    n, s = 65, 8
    rng = np.random.default_rng(7200)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    mins = np.empty((n, s), dtype=np.uint64)
    for i in range(n):
        keep = rng.random(s) < 0.5
        mins[i] = np.where(keep, base, rng.integers(0, 194481, size=s).astype(np.uint64))
    weights = -rng.gamma(2.0, 1e-3, size=(n, s))
    weights[rng.random((n, s)) < 0.05] *= -1
    fresh = (1 << 40) + np.arange(64, dtype=np.uint64)
    mins[X0] = fresh[0:8]; mins[X1] = np.concatenate([fresh[0:4], fresh[8:12]])
    weights[X0] = [1.0, -1.0, 1.0, -1.0, 0.01, 0.01, 0.01, 0.01]
    weights[X1] = [0.01, 0.01, 0.01, 0.01, -1.0, 1.0, -1.0, 1.0]
    mins[Y] = fresh[16:24]; mins[Z] = mins[Y]; weights[Z] = 0.0; weights[Z, ::2] = -0.0
    mins[U] = fresh[24:32]; mins[V] = np.concatenate([fresh[24:26], fresh[32:38]]); weights[U, 0] = np.inf
    mins[I1] = mins[I0]; weights[I1] = weights[I0]
    D = pyorc.smash_matrix(mins, weights, "weightedjaccard")
    for a in (mins, weights, D):
        a.setflags(write=False)
    return mins, weights, D


def check_weighted_set():
    mins, weights, D = weighted_set()
    tau = 0.5
    assert D[X0, X1] <= tau < D[X1, X0], NO_TEST + "the bridge links in both directions or in none"
    assert is_bridge(D, tau, (X0, X1)), NO_TEST + "(X0, X1) is no bridge"
    lab_or, lab_and = components(D, tau)[0], components(D, tau, rule="and")[0]
    assert lab_or[X1] == lab_or[X0] and lab_and[X1] != lab_and[X0] and not np.array_equal(lab_or, lab_and), NO_TEST + "the AND rule gives the same components"
    assert np.isnan(D[Z]).all() and D[Y, Z] == 0 and lab_or[Z] == lab_or[Y], NO_TEST + "the all-zero subject"
    assert np.isnan(D[U, V]) and D[U, I0] == 1 and np.isnan(D[U, U]), NO_TEST + "the Inf weight"
    assert D[I0, I1] == 0 and D[I1, I0] == 0 and np.array_equal(mins[I0], mins[I1]), NO_TEST + "the identical pair"
    at0, at1 = components(D, 0.0), components(D, 1.0)
    assert at0[0][I1] == I0 and at0[0][Z] == Y, NO_TEST + "tau = 0 does not link the identical sketches"
    assert at1[1] == int((~np.isnan(D)).sum() - (~np.isnan(np.diag(D))).sum()) and at1[2] == 1, NO_TEST + "tau = 1 does not link every non-NaN pair"
    return {t: components(D, t) for t in (0.0, 0.5, 1.0)}


@functools.lru_cache(maxsize=None)
def random_set(s):
    """257 sketches over a shared base (tests/test_gpu_panel.py's make_sketches) and, per metric, D and the thresholds at the 1 %,
    10 % and 50 % quantile of its off-diagonal distances (method "lower": a distance that occurs, so equality is exercised)"""
    n = 257
    rng = np.random.default_rng(7300 + s)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    mins = np.empty((n, s), dtype=np.uint64)
    for i in range(n):
        keep = rng.random(s) < (0.2 + 0.6 * rng.random())
        mins[i] = np.where(keep, base, rng.integers(0, 194481, size=s).astype(np.uint64))
    weights = -rng.gamma(2.0, 1e-3, size=(n, s))
    weights[rng.random((n, s)) < 0.05] *= -1
    out = {}
    for metric in ("jaccard", "weightedjaccard"):
        D = pyorc.smash_matrix(mins, weights, metric)
        off = D[~np.eye(n, dtype=bool)]
        taus = [float(np.quantile(off[~np.isnan(off)], q, method="lower")) for q in (0.01, 0.10, 0.50)]
        D.setflags(write=False)
        out[metric] = (D, taus)
    mins.setflags(write=False); weights.setflags(write=False)
    return mins, weights, out


def check_random_set(s):
    mins, weights, out = random_set(s)
    for metric, (D, taus) in out.items():
        assert all(0 <= t <= 1 for t in taus), NO_TEST + "a threshold outside [0, 1]"
        links = [components(D, t)[1] for t in taus]
        assert 0 < links[0] <= links[1] <= links[2] and links[2] >= 257 * 256 // 2, NO_TEST + f"{metric}: links {links}"
        if s > 8:
            assert components(D, taus[0])[2] > 1, NO_TEST + f"{metric}: the sparsest threshold already gives one cluster"


def bands_planned(n, band_rows):
    b = band_rows or 2048
    return (n + b - 1) // b
