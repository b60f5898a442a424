"""The three users of the pair tile (hulk_pairtile.h) agree with each other: k_smash's matrix, k_search_dist's lists and
k_cluster_link's links over ONE set of sketches.

N = 97 sketches: three subject tiles of 32 with a one-row tail, two tiles of 64 others, the second partial.  S = 33 (a chunk of 32
slots and a one-slot tail) and S = 1.  Both metrics.  The set comes from tests/test_gpu_panel.py's generator over a shared base,
as tests/test_gpu_search.py's inputs do; at S = 33 at least a third of the distances lie strictly inside (0, 1), which is asserted
(at S = 1 a distance is 0 or 1 whatever the input: 1 - w / w or 1 - 0 / w, 1 - 1 / 1 or 1 - 0 / 1).
The matrix hulk_smash returns is compared with the CPU oracle's once; everything else is compared with that matrix, bit for bit."""
import functools

import numpy as np
import pytest

import cluster_inputs as ci
from oracle import pyorc
from test_gpu_cluster import assert_same, run
from test_gpu_panel import make_sketches
from test_gpu_search import assert_hits, bits, select

pytestmark = pytest.mark.gpu

N, K = 97, 64
METRICS = ("jaccard", "weightedjaccard")
CASES = [(s, metric) for s in (33, 1) for metric in METRICS]


@functools.lru_cache(maxsize=None)
def sketches(s):
    rng = np.random.default_rng(9700 + s)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    mins, weights = make_sketches(rng, N, s, base)
    mins.setflags(write=False); weights.setflags(write=False)
    return mins, weights


@functools.lru_cache(maxsize=None)
def matrix(s, metric):
    """hulk_smash's matrix of the set, checked against the oracle's and for being a test at all"""
    from hulk_amd.smash import distance_matrix
    mins, weights = sketches(s)
    D = distance_matrix(mins, weights, metric)
    want = pyorc.smash_matrix(mins, weights, metric)
    bad = np.argwhere(bits(D) != bits(want))
    assert len(bad) == 0, f"S {s} {metric}: {len(bad)} entries of hulk_smash's matrix differ from the oracle's, first at {bad[0].tolist()}: got {D[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"
    assert not np.isnan(D).any()
    inner = int(((D > 0) & (D < 1)).sum())
    print(f"S {s} {metric}: {inner} of {D.size} distances strictly inside (0, 1)")
    if s > 1:
        assert 3 * inner >= D.size, "the inputs are no test: too few distances strictly between 0 and 1"
    D.setflags(write=False)
    return D


def by_role(D, role):
    """row i of the result = the distances a self search of query i selects from: its row of the matrix, or its column"""
    return D if role == "row" else np.ascontiguousarray(D.T)


@pytest.mark.parametrize("s,metric", CASES)
def test_self_search_is_the_selection_from_the_matrix(s, metric):
    from hulk_amd.smash import search
    mins, weights = sketches(s)
    D = matrix(s, metric)
    for role in ("row", "column"):
        got = search(mins, weights, None, None, K, metric, role, self_search=True)
        assert_hits(got, select(by_role(D, role), K, no_diagonal=True), f"N {N} S {s} K {K} {metric} {role} self")


@pytest.mark.parametrize("s,metric", CASES)
def test_cluster_is_the_graph_of_the_matrix(s, metric):
    mins, weights = sketches(s)
    D = matrix(s, metric)
    tau = float(np.median(D[~np.eye(N, dtype=bool)]))
    want = ci.components(D, tau)
    assert want[1] == int(((D <= tau) & ~np.eye(N, dtype=bool)).sum())
    print(f"S {s} {metric}: tau {tau!r}, {want[1]} links, {want[2]} clusters")
    for band in (32, 0):
        assert_same(run(mins, weights, tau, metric, band), want, f"N {N} S {s} {metric} band_rows {band} tau {tau!r}")


@pytest.mark.parametrize("s,metric", CASES)
def test_query_blocks_of_32_read_the_padding_and_change_nothing(s, metric):
    """role column with query blocks of 32: the 64-wide tile of other columns that starts at query 96 runs 32 doubles past every
    slot's row of the prepared queries (128 columns), behind the last slot into the + 64 doubles hulk_search pads them with
    (weighted jaccard; for jaccard the two roles are one kernel, whose subjects are the queries)"""
    from hulk_amd.smash import search
    mins, weights = sketches(s)
    D = matrix(s, metric)
    one, many = {}, {}
    a = search(mins, weights, None, None, K, metric, "column", self_search=True, stats=one)
    b = search(mins, weights, None, None, K, metric, "column", self_search=True, scratch_bytes=64 * (s * 32 + 32 * 8), stats=many)
    assert one["query_blocks"] == 1, one
    assert many["query_blocks"] > 1 and many["query_blocks"] == (N + 31) // 32, many     # blocks of 32 queries
    assert_hits(b, select(by_role(D, "column"), K, no_diagonal=True), f"N {N} S {s} K {K} {metric} column self, {many['query_blocks']} query blocks")
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
