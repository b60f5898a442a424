"""hulk_cluster, hulk_dendrogram and hulk_links at N = 4161 (tests/scale_inputs.py): thousands of workgroups a launch, several to a
CU and most of them started after others have finished — the load under which k_cluster_link's lock-free union-find has to hold —,
and the first size at which k_dendro_fold's two strided loops take a second and a third trip.

The yardstick is the oracle's matrix over the whole set (jaccard, weighted jaccard) or, for bottomk, the GPU's own matrix held to
bottomk_inputs.matrix on a 64-sketch sample; test_matrix_anchor compares distance_matrix with it bit for bit and everything else
goes from that matrix through cluster_inputs.components, dendrogram_inputs.kruskal / cut_labels and links_inputs.csr.  Every
"the inputs are no test" condition is asserted before anything is compared."""
import functools

import numpy as np
import pytest

import bottomk_inputs as bi
import cluster_inputs as ci
import dendrogram_inputs as di
import links_inputs as li
import scale_inputs as sc
from test_gpu_cluster import assert_same as assert_same_clusters, run as run_cluster
from test_gpu_dendrogram import assert_same as assert_same_edges, run as run_dendrogram
from test_gpu_links import run as run_links

pytestmark = pytest.mark.gpu

CASES = [(name, metric) for name in sorted(sc.SETS) for metric in sc.METRICS]


def arrays(name, metric):
    mins, weights = sc.SETS[name]()[:2]
    return mins, (None if metric == "bottomk" else weights)


@functools.lru_cache(maxsize=None)
def yardstick(name, metric):
    """the matrix everything is compared with, anchored: the GPU's equals the oracle's in every bit (bottomk: on the sample, and it
    is symmetric with a zero diagonal)"""
    from hulk_amd.smash import distance_matrix
    mins, weights = arrays(name, metric)
    G = distance_matrix(mins, weights, metric)
    assert G.shape == (sc.N, sc.N) and G.dtype == np.float64
    if metric in sc.ORACLE_METRICS:
        D = sc.matrix(name, metric)
        bad = np.argwhere(di.bits(G) != di.bits(D))
        assert len(bad) == 0, f"{name} {metric}: {len(bad)} entries differ from the oracle's, first at {bad[:3].tolist()}"
        return D
    idx = sc.sample_rows(name)
    assert len(idx) == sc.SAMPLE == len(set(idx.tolist()))
    want = bi.matrix(mins[idx])
    assert np.array_equal(di.bits(G[np.ix_(idx, idx)]), di.bits(want)), f"{name} bottomk: the sampled sub-matrix differs from the yardstick's"
    assert np.array_equal(di.bits(G), di.bits(G.T)) and not np.diag(G).any() and not np.isnan(G).any()
    return sc.give_matrix(name, metric, G)


# ---- 1. the anchor -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,metric", CASES)
def test_matrix_anchor(name, metric):
    D = yardstick(name, metric)
    if metric != "weightedjaccard":
        assert np.array_equal(D, D.T)
    print(f"{name} {metric}: {int((D < 1.0).sum()) - sc.N} off-diagonal distances below 1.0 of {sc.N * (sc.N - 1)}")


@pytest.mark.parametrize("order", sc.ORDERS)
def test_matrix_anchor_of_the_one_chain(order):
    from hulk_amd.smash import distance_matrix
    mins, weights, D = sc.one_chain(order)
    assert np.array_equal(di.bits(distance_matrix(mins, weights, "jaccard")), di.bits(D))


# ---- 2. cluster --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", sc.METRICS)
def test_cluster_chains(metric):
    """five chains and 61 singletons under three thresholds and three band plans: the union-find under thousands of workgroups,
    no flatten between the three default bands, a hook per band with 131 bands; twice, byte-equal"""
    yardstick("chains", metric)
    facts = sc.check_chains("chains", metric)
    mins, weights = arrays("chains", metric)
    for tau in sc.thresholds("chains", metric):
        want = sc.clustering("chains", metric, tau)
        print(f"chains {metric} tau {tau!r}: {facts[tau][0]} links, {facts[tau][1]} clusters")
        for band in sc.CLUSTER_BANDS:
            got = run_cluster(mins, weights, tau, metric, band)
            assert_same_clusters(got, want, f"chains {metric} tau {tau!r} band_rows {band}")
            again = run_cluster(mins, weights, tau, metric, band)
            assert again[0].tobytes() == got[0].tobytes() and again[1:] == got[1:], f"chains {metric} tau {tau!r} band_rows {band}: a second call differs"


@pytest.mark.parametrize("order", sc.ORDERS)
def test_cluster_one_chain(order):
    """4160 bridges: one lost union splits the component; one ulp below nothing links"""
    mins, weights, D = sc.one_chain(order)
    want = sc.check_one_chain(order)
    below = float(np.nextafter(sc.TAU, 0.0))
    for band in sc.CLUSTER_BANDS:
        got = run_cluster(mins, weights, sc.TAU, "jaccard", band)
        assert_same_clusters(got, want, f"{order} band_rows {band}")
        assert not got[0].any() and got[2] == 1 and got[1] == 2 * (sc.N - 1)
        assert run_cluster(mins, weights, sc.TAU, "jaccard", band)[0].tobytes() == got[0].tobytes()
        got = run_cluster(mins, weights, below, "jaccard", band)
        assert_same_clusters(got, sc.chain_clustering(order, True), f"{order} band_rows {band}, one ulp below")
        assert got[2] == sc.N and got[1] == 0 and np.array_equal(got[0], np.arange(sc.N))


# ---- 3. dendrogram -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,metric", CASES)
def test_dendrogram(name, metric):
    """far_pairs: sketches whose nearest partner only the second (third) trip of a fold loop sees, in the row partials and in the
    column partials (scale_inputs.GROUPS); chains: ties everywhere.  The edges are Kruskal's, the cut at chain_tau(8) is the
    clustering of the same set"""
    from hulk_amd.smash import cluster, cut_dendrogram
    D = yardstick(name, metric)
    if name == "far_pairs":
        witnesses = sc.check_far_pairs(metric)
        print(f"far_pairs {metric}: witnesses {({k: len(v) for k, v in witnesses.items()})}")
    sc.check_chains(name, metric)
    mins, weights = arrays(name, metric)
    want = sc.forest(name, metric)
    labels = sc.clustering(name, metric, sc.TAU)[0]
    clustered = cluster(mins, weights, sc.TAU, metric)
    assert np.array_equal(clustered[0], labels)
    for band in sc.DENDRO_BANDS:
        got, st = run_dendrogram(mins, weights, metric, band)
        assert_same_edges(got, want, f"{name} {metric} band_rows {band}")
        assert st["rounds"] <= di.round_bound(sc.N), st
        if (name, metric) == sc.ROUNDS_CASE:
            assert st["rounds"] == sc.rounds(name, metric), (st, sc.rounds(name, metric))
        cut = cut_dendrogram(sc.N, *got, sc.TAU)
        assert np.array_equal(cut[0], clustered[0]) and cut[1] == clustered[1], f"{name} {metric} band_rows {band}: the cut is not the clustering"
        assert np.array_equal(di.cut_labels(sc.N, *got, sc.TAU), labels)


# ---- 4. links ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", sc.METRICS)
def test_links_chains(metric):
    from hulk_amd.smash import cluster
    D = yardstick("chains", metric)
    sc.check_chains("chains", metric)
    mins, weights = arrays("chains", metric)
    want = {upper: li.csr(D, sc.TAU, upper=upper) for upper in (False, True)}
    assert 0 < int(want[True][0][-1]) < int(want[False][0][-1]) == sc.clustering("chains", metric, sc.TAU)[1]
    assert int(want[False][0][2048]) not in (0, int(want[False][0][-1])) and int(want[False][0][4096]) != int(want[False][0][-1]), ci.NO_TEST + "a default band without a link"
    for band in sc.LINKS_BANDS:
        for upper in (False, True):
            got = run_links(mins, weights, sc.TAU, metric, band, upper=upper)
            li.assert_same(got, want[upper], f"chains {metric} band_rows {band} upper {upper}")
    ptr, idx, _ = got = run_links(mins, weights, sc.TAU, metric)
    rows = np.repeat(np.arange(sc.N), li.degrees(ptr))
    labels, n_clusters = cluster(mins, weights, sc.TAU, metric)
    assert np.array_equal(ci.union_find_labels(sc.N, zip(rows.tolist(), idx.tolist())), labels), f"{metric}: a union-find over the listed edges gives cluster's labels"
    assert np.array_equal(labels, sc.clustering("chains", metric, sc.TAU)[0]) and 1 < n_clusters < sc.N
