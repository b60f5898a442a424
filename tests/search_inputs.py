"""The yardstick of the search tests (tests/test_gpu_search.py, tests/test_search_cpu.py) and the inputs that take k_search_select
beyond one pass of a strip's row; no test lives here.

The yardstick is oracle.pyorc.smash_matrix over the stack [queries; database] — block [:m, m:] for role "row", [m:, :m].T for role
"column" — then the selection in numpy: mask NaN and the values above max_distance, np.lexsort((index, distance)), the first K.

k_search_select reads a row 64 * SELECT_AHEAD = 512 distances a pass.  The inputs here are five queries against up to 1100 database
sketches — strips that end one short of, at and one behind the first and the second pass, and 1100: a third pass with a tail — at
S = 8 under jaccard, where ties abound and the index decides, and S = 33 under weightedjaccard, where distances are mostly distinct.
Every check_* function asserts on the yardstick alone that an input exercises what it claims ("the inputs are no test")."""
import bisect
import functools
import os
import re

import numpy as np

from oracle import pyorc
from test_gpu_panel import make_sketches            # (a generator: a base shared between the two sides, so that equal slots exist across them)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
NO_TEST = "the inputs are no test: "


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def blocks(qm, qw, dm, dw, metric):
    """one call of the yardstick over [queries; database] -> {"row": [m][P], "column": [m][P]}"""
    m = len(qm)
    full = pyorc.smash_matrix(np.vstack([qm, dm]), np.vstack([qw, dw]), metric)
    return {"row": np.ascontiguousarray(full[:m, m:]), "column": np.ascontiguousarray(full[m:, :m].T)}


def blocks_few_queries(qm, qw, dm, dw, metric, chunk=128):
    """blocks() for a handful of queries against a long database: the yardstick a chunk of the database at a time (a pair's distance
    depends on the pair alone), so that the database's own pairs are not computed"""
    parts = [blocks(qm, qw, dm[a:a + chunk], dw[a:a + chunk], metric) for a in range(0, len(dm), chunk)]
    return {role: np.ascontiguousarray(np.hstack([p[role] for p in parts])) for role in ("row", "column")}


def select(D, k, max_distance=None, no_diagonal=False):
    """the hit lists of the issue's rule, from the distances [m][P]"""
    m, P = D.shape
    index = np.full((m, k), NONE, dtype=np.uint32); dist = np.full((m, k), np.nan); count = np.zeros(m, dtype=np.uint32)
    for i in range(m):
        ok = ~np.isnan(D[i])
        if max_distance is not None and 0 <= max_distance <= 1:
            ok &= D[i] <= max_distance
        if no_diagonal:
            ok[i] = False
        cand = np.nonzero(ok)[0]
        order = cand[np.lexsort((cand, D[i][cand]))][:k]
        count[i] = len(order); index[i, :len(order)] = order; dist[i, :len(order)] = D[i][order]
    return index, dist, count


# ---- the long strips -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pass_length():
    """the distances of a row that k_search_select reads in one pass: 64 * SELECT_AHEAD, from the source"""
    text = open(os.path.join(ROOT, "hulk_amd", "csrc", "hulk_search.hip")).read()
    return 64 * int(re.search(r"constexpr int SELECT_AHEAD = (\d+);", text).group(1))


LONG_M, LONG_P, LONG_K = 5, 1100, 64
LONG_PS = (511, 512, 513, 1023, 1024, 1025, 1100)
LONG_KS = (1, 2, 33, 63, 64)
LONG_CASES = ((8, "jaccard"), (33, "weightedjaccard"))          # ties abound / distances mostly distinct
ROLES = ("row", "column")
STRIP = 576                                                     # "more than one long strip": 576 + 524 sketches, both longer than a pass
ORDERS = ("descending", "ascending", "identical", "copies")
COPIES = tuple(range(509, 516))                                 # a run of equal keys across the border of the first pass


def strip_scratch(s, mb=32):
    """the scratch_bytes at which search_plan gives strips of STRIP sketches: Pb = scratch / (32 * S + 8 * Mb), down to a multiple of 64"""
    assert STRIP % 64 == 0
    return STRIP * (32 * s + 8 * mb)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def long_inputs(s):
    """(qm, qw, dm, dw): 5 queries and 1100 database sketches of s slots over a shared base; every P < 1100 is a prefix of the database"""
    rng = np.random.default_rng(5100 + s)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    qm, qw = make_sketches(rng, LONG_M, s, base)
    dm, dw = make_sketches(rng, LONG_P, s, base)
    # the first sketch of the second pass is query 1 itself and the first of the third pass query 2: hit 0 of those queries at every K,
    # the only candidate of its pass at P = 513 and P = 1025
    n = pass_length()
    dm[n], dw[n], dm[2 * n], dw[2 * n] = qm[1], qw[1], qm[2], qw[2]
    return frozen(qm, qw, dm, dw)


@functools.lru_cache(maxsize=None)
def long_blocks(s, metric):
    qm, qw, dm, dw = long_inputs(s)
    b = blocks_few_queries(qm, qw, dm, dw, metric)
    frozen(*b.values())
    return b


def thinned(role):
    """the (P, K) pairs a role runs: every other one, the other role the rest — each K meets every P, and each role every K and P"""
    r = ROLES.index(role)
    return [(p, k) for j, p in enumerate(LONG_PS) for i, k in enumerate(LONG_KS) if (i + j + r) % 2 == 0]


def check_long_strips(s, metric):
    n = pass_length()
    assert n == 512, "SELECT_AHEAD moved: look at what LONG_PS, STRIP and COPIES straddle"
    assert {n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1} < set(LONG_PS) and max(LONG_PS) == LONG_P > 2 * n + 64
    assert n < LONG_P - STRIP < STRIP and (LONG_P - STRIP) % 64, NO_TEST + "the second strip has no second pass with a tail"
    assert min(COPIES) < n <= max(COPIES)
    assert {1, 2, 33, 63, 64} == set(LONG_KS)
    pairs = {pk for role in ROLES for pk in thinned(role)}
    assert pairs == {(p, k) for p in LONG_PS for k in LONG_KS}, NO_TEST + "a K never meets a P"
    for role in ROLES:
        assert {p for p, _ in thinned(role)} == set(LONG_PS) and {k for _, k in thinned(role)} == set(LONG_KS)
    for role in ROLES:
        D = long_blocks(s, metric)[role]
        assert D.shape == (LONG_M, LONG_P) and not np.isnan(D).all(axis=1).any()
        inner = ((D > 0) & (D < 1)).mean()
        assert inner > 1 / 3, NO_TEST + f"{inner:.2f} of the distances lie strictly between 0 and 1"
        srt = np.sort(D, axis=1)
        if metric == "jaccard":                                     # the tie-break by index decides the answer
            assert all((srt[:, k - 1] == srt[:, k]).mean() >= 0.6 for k in LONG_KS), NO_TEST + "the tie-break by index decides nothing"
        else:
            assert len(np.unique(D[0][~np.isnan(D[0])])) > LONG_P // 2, NO_TEST + "weighted distances tie"
        # hits behind the first and behind the second pass, so that gi = pbase + c with c >= 512 and c >= 1024 is reported
        for p, k in thinned(role):
            idx = select(D[:, :p], k)[0]
            assert p <= n or idx[1, 0] == n, NO_TEST + f"P {p} K {k}: the first sketch of the second pass is not query 1's hit 0"
            assert p <= 2 * n or idx[2, 0] == 2 * n, NO_TEST + f"P {p} K {k}: the first sketch of the third pass is not query 2's hit 0"


def insertions(drow, k):
    """replays the selection of one query over its row in index order: how many candidates enter the list of the k best keys
    (distance, index) at the moment they are seen"""
    held, entered = [], 0
    for i, d in enumerate(drow.tolist()):
        if d != d:
            continue
        key = (d, i)
        if len(held) < k or key < held[-1]:
            bisect.insort(held, key)
            del held[k:]
            entered += 1
    return entered


@functools.lru_cache(maxsize=None)
def ordered_database(s, metric, role, order):
    """(dm, dw, D [5][1100]): the database in an order made for query 0.
    descending / ascending: sorted by the distance to query 0 (NaN last) — every candidate enters at rank 0 / none enters after the
    first K; identical: 1100 copies of one sketch, every key ties; copies: the random set with the sketches 509 .. 515 replaced by
    copies of query 0's nearest sketch, a run of equal distances across the border of the first pass"""
    qm, qw, dm, dw = long_inputs(s)
    D0 = long_blocks(s, metric)[role][0]
    if order in ("descending", "ascending"):
        by = np.lexsort((np.arange(LONG_P), np.where(np.isnan(D0), np.inf, D0)))      # ascending, NaN last
        valid = int((~np.isnan(D0)).sum())
        perm = by if order == "ascending" else np.concatenate([by[:valid][::-1], by[valid:]])
        dm, dw = dm[perm], dw[perm]
    elif order == "identical":
        near = int(select(D0[None, :], 1)[0][0, 0])
        dm, dw = np.repeat(dm[near:near + 1], LONG_P, axis=0), np.repeat(dw[near:near + 1], LONG_P, axis=0)
    else:
        near = int(select(D0[None, :], 1)[0][0, 0])
        dm, dw = dm.copy(), dw.copy()
        dm[list(COPIES)] = dm[near]; dw[list(COPIES)] = dw[near]
    dm, dw = np.ascontiguousarray(dm), np.ascontiguousarray(dw)
    D = blocks_few_queries(qm, qw, dm, dw, metric)[role]
    return frozen(dm, dw, D)


def check_orders(s, metric, role):
    n = pass_length()
    D0 = long_blocks(s, metric)[role][0]
    valid = int((~np.isnan(D0)).sum())
    assert valid > LONG_P - 64
    out = {}
    for order in ORDERS:
        D = ordered_database(s, metric, role, order)[2]
        entered = out[order] = insertions(D[0], LONG_K)
        index, dist, count = select(D, LONG_K)
        if order == "descending":
            assert (np.diff(D[0][:valid]) <= 0).all()
            if metric == "weightedjaccard":
                assert 2 * entered >= LONG_P, NO_TEST + f"{entered} of {LONG_P} candidates enter query 0's list"
            else:                                                   # (equal distances arrive in ascending index: a tie never enters a full list)
                assert entered >= LONG_K + len(np.unique(D[0][:valid])) - 1
        elif order == "ascending":
            assert (np.diff(D[0][:valid]) >= 0).all() and entered == LONG_K, NO_TEST + f"{entered} candidates enter in ascending order"
            assert index[0].tolist() == list(range(LONG_K))
        elif order == "identical":
            assert len(np.unique(bits(D[0]))) == 1 and not np.isnan(D[0, 0]), NO_TEST + "the identical sketches are not at one distance"
            assert (index == np.arange(LONG_K, dtype=np.uint32)[None, :]).all() and (count == LONG_K).all()
            assert all(len(np.unique(bits(D[q]))) == 1 for q in range(LONG_M))
        else:
            near = int(select(D0[None, :], 1)[0][0, 0])
            assert near not in COPIES
            # the sketches at query 0's smallest distance: the copies and their original (under jaccard a few more), all of them hits,
            # in index order, on both sides of the border
            group = np.flatnonzero(D[0] == np.nanmin(D[0])).tolist()
            assert set(COPIES + (near,)) <= set(group) and len(group) < LONG_K, NO_TEST + "the copies are not query 0's nearest"
            assert index[0, :len(group)].tolist() == group and dist[0, len(group)] > dist[0, 0]
            assert sum(g < n for g in group) >= 3 and sum(g >= n for g in group) >= 3
    return out


# ---- self search and a distance limit at N = 1100 ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def self_blocks(s, metric):
    _, _, dm, dw = long_inputs(s)
    full = pyorc.smash_matrix(dm, dw, metric)
    b = {"row": np.ascontiguousarray(full), "column": np.ascontiguousarray(full.T)}
    frozen(*b.values())
    return b


def self_limit(s, metric, role):
    """a max_distance below which 2 % of the pairs lie: for the queries it leaves fewer than K hits it is the limit — not the K-th key
    — that rejects the candidates of every pass"""
    D = self_blocks(s, metric)[role]
    off = D[~np.eye(LONG_P, dtype=bool)]
    return float(np.quantile(off[~np.isnan(off)], 0.02, method="lower"))


def check_self_search(s, metric, role):
    n = pass_length()
    D = self_blocks(s, metric)[role]
    lim = self_limit(s, metric, role)
    assert 0 < lim < 1
    index, dist, count = select(D, LONG_K, max_distance=lim, no_diagonal=True)
    cut = (count > 0) & (count < LONG_K)
    # (a sketch keeps between 0.2 and 0.8 of the shared base, so one limit leaves the sparse ones no hit and the dense ones a full list;
    # a hundred lists in between, cut by the limit alone and with hits on both sides of the first pass, are what the test needs)
    both = [q for q in np.nonzero(cut)[0] if (index[q, :count[q]] < n).any() and (index[q, :count[q]] >= n).any()]
    assert len(both) >= 100, NO_TEST + f"{len(both)} lists cut by the limit with hits on both sides of the first pass"
    # ... and inside the second pass the limit accepts some candidates of such a list and rejects others
    second = D[both][:, n:2 * n]
    assert ((second <= lim).any(axis=1) & (second > lim).any(axis=1)).sum() >= 100, NO_TEST + "the limit does not cut inside the second pass"
    free = select(D, LONG_K, no_diagonal=True)
    assert (free[2] == LONG_K).all() and (free[0][:, -1] >= 0).all()
    return lim, (index, dist, count), free
