"""The inputs of tests/test_gpu_collection_scale.py are a test: every check_* of tests/scale_inputs.py on the oracle's matrices (jaccard,
weighted jaccard; the bottomk matrix comes from the GPU and the GPU tests run the same checks on it), and the early exit of
dendrogram_inputs.kruskal against the loop without it.  No device."""
import numpy as np
import pytest

import cluster_inputs as ci
import dendrogram_inputs as di
import scale_inputs as sc


def test_the_shape_is_past_the_first_trip_of_both_fold_loops():
    assert sc.N == 65 * 64 + 1 and (sc.N + 63) // 64 == 66 and (sc.N + 31) // 32 == 131
    assert (sc.N + 63) // 64 - 0 > 64, ci.NO_TEST + "the row loop of k_dendro_fold takes one trip"
    for band, tiles in ((2080, 65), (4192, 131)):
        assert (min(band, sc.N) + 31) // 32 == tiles > 64 and band % 32 == 0
    assert [ci.bands_planned(sc.N, b) for b in sc.CLUSTER_BANDS] == [3, 131, 1]
    assert sum(sc.CHAIN_SIZES) + 61 == sc.N and sc.TAU == 0.25 and len(sc.RESERVED) == 30
    mins, weights, D, members = sc.chains()
    assert int(mins.max()) < 1 << 50 and (weights < 0).all() and sorted(len(m) for m in members) == sorted(sc.CHAIN_SIZES)
    assert len({i for m in members for i in m}) == sum(sc.CHAIN_SIZES)
    assert not set(sc.RESERVED) & {i for m in sc.far_pairs()[3] for i in m}, ci.NO_TEST + "a planted sketch overwrote a chain member"


@pytest.mark.parametrize("metric", sc.ORACLE_METRICS)
def test_far_pairs_need_the_later_trips(metric):
    out = sc.check_far_pairs(metric)
    print(metric, {k: len(v) for k, v in out.items()})


@pytest.mark.parametrize("metric", sc.ORACLE_METRICS)
@pytest.mark.parametrize("name", sorted(sc.SETS))
def test_chains_link_something_and_not_everything(name, metric):
    out = sc.check_chains(name, metric)
    print(name, metric, {repr(tau): v for tau, v in out.items()})
    assert sc.thresholds(name, metric)[0] == sc.TAU
    if metric == "weightedjaccard":
        assert len(sc.thresholds(name, metric)) == 3, ci.NO_TEST + "the quantiles coincide"


def test_the_offer_form_takes_several_rounds_and_is_kruskal():
    print("rounds", sc.rounds(*sc.ROUNDS_CASE))


@pytest.mark.parametrize("order", sc.ORDERS)
def test_one_chain_is_held_by_bridges(order):
    sc.check_one_chain(order)
    mins = sc.one_chain(order)[0]
    if order != "random":
        assert (mins[0] != mins[1]).sum() == sc.T0 and (mins[0] != mins[2]).sum() == 2 * sc.T0, "index neighbours are chain neighbours"


def kruskal_without_exit(D):
    """dendrogram_inputs.kruskal as it was before its early exit: every edge is visited"""
    W = di.edge_weights(np.asarray(D, dtype=np.float64))
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
    for x, y, h in zip(i[order].tolist(), j[order].tolist(), w[order].tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
            a.append(x); b.append(y); d.append(h)
    return np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32), np.array(d, dtype=np.float64)


def test_kruskal_with_its_early_exit_is_kruskal():
    """on the planted chains (a tree), on the weighted set (NaN directions) and on a forest that never reaches n - 1 edges"""
    mins, weights, D, members = ci.planted_chains(8)
    sets = [D["jaccard"], D["weightedjaccard"], ci.weighted_set()[2]]
    split = np.array(D["weightedjaccard"])
    split[:100, 100:] = np.nan; split[100:, :100] = np.nan            # two components: the loop runs to its end
    sets.append(split)
    for M in sets:
        got, want = di.kruskal(M), kruskal_without_exit(M)
        assert di.same_edges(got, want) and got[0].dtype == want[0].dtype and got[2].dtype == want[2].dtype
    assert len(di.kruskal(split)[0]) == 255
    # past one piece of 2^16 edges with edges left over: the exit is taken and changes nothing
    J = sc.one_chain("random")[2][:600, :600]
    assert di.same_edges(di.kruskal(J), kruskal_without_exit(J)) and 600 * 599 // 2 > 1 << 16
