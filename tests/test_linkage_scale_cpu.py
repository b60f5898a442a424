"""The inputs and the yardstick of tests/test_gpu_linkage_scale.py are a test (tests/linkage_scale_inputs.py): the cached yardstick
gives the literal one's merges on every set the small suite uses and on the first 600 sketches of every set here; every size follows
LINK_CHUNK as hulk_linkage.hip states it; every check_* holds on the oracle's matrices (the bottomk cases get theirs from the GPU, and
the GPU tests run the same checks on them); the three cluster-pair identities hold on the literal yardstick's output.  No device."""
import numpy as np
import pytest

import bottomk_inputs as bk
import cluster_inputs as ci
import linkage_inputs as li
import linkage_scale_inputs as ls
import scale_inputs as sc

SMALL_SETS = [(kind, arg, metric) for kind, arg in li.JACCARD_SETS for metric in li.METRICS]
SMALL_SETS += [(kind, None, metric) for kind in ("identical_set", "disjoint_set") for metric in li.METRICS]
SMALL_SETS += [("zero_weight_set", None, "weightedjaccard")]


def assert_agree(D, what):
    for method in li.METHODS:
        got, want = ls.agglomerate_cached(D, method), li.agglomerate(D, method)
        assert li.same_merges(got, want), f"{what} {method}: the cached yardstick is not the literal one"
        assert [x.dtype for x in got] == [x.dtype for x in want]


@pytest.mark.parametrize("kind,arg,metric", SMALL_SETS)
def test_the_cached_yardstick_is_the_literal_one_on_the_small_suites_sets(kind, arg, metric):
    D = li.named_set(kind, arg, metric)[2]
    for method in li.METHODS:
        got = ls.agglomerate_cached(D, method)
        assert li.same_merges(got, li.reference(kind, arg, metric, method)), f"{kind}({arg}) {metric} {method}"
        assert [x.dtype.name for x in got] == ["uint32", "uint32", "float64", "uint32"]


def test_the_cached_yardstick_is_the_literal_one_on_the_forest_the_stars_and_bottomk():
    assert_agree(li.weighted_forest_set()[2], "weighted_forest_set")
    assert_agree(bk.matrix(bk.random_set(70, 16, 4100)), "the bottomk set")
    for kind, arg in (("random_set", 33), ("planted_chains", 8)):    # the prefixes test_gpu_linkage.py's shapes use
        D = li.named_set(kind, arg, "weightedjaccard")[2]
        for n in ci.NS:
            assert_agree(D[:n, :n], f"{kind}({arg}) N {n}")
    for method in li.METHODS:
        assert [len(x) for x in ls.agglomerate_cached(np.zeros((1, 1)), method)] == [0] * 4
        assert [len(x) for x in ls.agglomerate_cached(np.full((3, 3), np.nan), method)] == [0] * 4


@pytest.mark.parametrize("name", ["dense", "chains", "border", "inside"])
def test_the_cached_yardstick_is_the_literal_one_on_the_first_600_sketches_of_the_new_sets(name):
    for metric in (sc.ORACLE_METRICS if name in ("dense", "chains") else ("weightedjaccard",)):
        D = ls.matrix(name, metric)[:ls.PREFIX, :ls.PREFIX]
        assert_agree(D, f"{name} {metric} N {ls.PREFIX}")
        if name in ("border", "inside"):
            z = ls.zeroed(name)
            assert 2 <= int((z < ls.PREFIX).sum()) and len(li.agglomerate(D, "complete")[0]) == ls.PREFIX - int((z < ls.PREFIX).sum())
    far = sc.far_pairs()[2]
    for metric in sc.ORACLE_METRICS if name == "chains" else ():
        assert_agree(far[metric][:ls.PREFIX, :ls.PREFIX], f"far_pairs {metric} N {ls.PREFIX}")


def test_a_hand_worked_forest_of_six_sketches():
    """0 and 5 have no distance to each other (NaN both ways); 5 has no row of its own, everybody reaches it through theirs.
    W: (0,1) 0.1  (0,2) 0.4  (0,3) 0.6  (0,4) 0.9  (0,5) inf  (1,2) 0.4  (1,3) 0.8  (1,4) 0.7  (1,5) 0.5  (2,3) 0.2  (2,4) 0.9
    (2,5) 0.3  (3,4) 0.9  (3,5) 0.3  (4,5) 0.2"""
    nan = float("nan")
    D = np.array([[0.0, 0.1, 0.4, 0.6, 0.9, nan],
                  [0.3, 0.0, 0.4, 0.8, 0.7, 0.5],
                  [0.4, 0.9, 0.0, 0.2, 0.9, 0.3],
                  [0.6, 0.8, 0.2, 0.0, 0.9, 0.3],
                  [0.9, 0.7, 0.9, 0.9, 0.0, 0.2],
                  [nan, nan, nan, nan, nan, nan]])
    # complete: (0,1) 0.1; (2,3) 0.2 before (4,5) 0.2 (the smaller pair); then {0,1}-{2,3} = 0.8 against {2,3}-{4,5} = 0.9 and
    # {0,1}-{4,5} = inf: (0,2) at 0.8; {0,1,2,3}-{4,5} holds the pair (0,5): +inf, two clusters stay
    a, b, d, s = ls.agglomerate_cached(D, "complete")
    assert (a.tolist(), b.tolist(), d.tolist(), s.tolist()) == ([0, 2, 4, 0], [1, 3, 5, 2], [0.1, 0.2, 0.2, 0.8], [2, 2, 2, 4])
    # average: {0,1}-{2,3}: d(0,2) = (0.4 + 0.4) / 2, d(0,3) = (0.6 + 0.8) / 2, then (1 * 0.4 + 1 * 0.7) / 2 against
    # {2,3}-{4,5}: d(2,4) = (0.9 + 0.9) / 2, d(2,5) = (0.3 + 0.3) / 2, d(2,{4,5}) = (0.9 + 0.3) / 2 = 0.6
    d02, d03 = (1.0 * 0.4 + 1.0 * 0.4) / 2.0, (1.0 * 0.6 + 1.0 * 0.8) / 2.0
    h = (1.0 * d02 + 1.0 * d03) / 2.0
    assert h < (1.0 * ((1.0 * 0.9 + 1.0 * 0.9) / 2.0) + 1.0 * ((1.0 * 0.3 + 1.0 * 0.3) / 2.0)) / 2.0
    a, b, d, s = ls.agglomerate_cached(D, "average")
    assert (a.tolist(), b.tolist(), d.tolist(), s.tolist()) == ([0, 2, 4, 0], [1, 3, 5, 2], [0.1, 0.2, 0.2, h], [2, 2, 2, 4])
    # single: one tree — 5 is reached through 4, 2 and 3; (2,5) 0.3 joins {2,3} and {4,5}, then (0,2) at 0.4
    st = {}
    a, b, d, s = ls.agglomerate_cached(D, "single", st)
    assert (a.tolist(), b.tolist(), d.tolist(), s.tolist()) == ([0, 2, 4, 2, 0], [1, 3, 5, 4, 2], [0.1, 0.2, 0.2, 0.3, 0.4], [2, 2, 2, 4, 6])
    # rows scanned: the first fill's 6, then row p and the live rows whose cached column was p or q — (0,1): row 0; (2,3): 2, and 0
    # (its nearest was 2 at 0.4); (4,5): 4, and 2 (its nearest was 5 at 0.3); (2,4): 2, and 0 (2 again); (0,2): 0
    assert st["rows_rescanned"] == 6 + 1 + 2 + 2 + 2 + 1
    for method in li.METHODS:
        assert li.same_merges(ls.agglomerate_cached(D, method), li.agglomerate(D, method))


def test_the_sizes_follow_link_chunk():
    assert ls.C == ls.link_chunk() == 4096, "LINK_CHUNK moved: the sizes below are derived from it, and DESIGN 4i names the value"
    assert ls.FULL_NS == (ls.C, ls.C + 1, ls.C + 2, sc.N) and sorted(ls.BORDER) == [ls.C - 1, ls.C, ls.C + 1]
    ls.check_sizes()
    wanted = {ls.wanted_merges(c) for c in ls.ORACLE_CASES + ls.BOTTOMK_CASES}
    assert {ls.C - 1, ls.C, ls.C + 1, sc.N - 1, ls.KEPT} == wanted
    assert len(set(ls.ORACLE_CASES + ls.BOTTOMK_CASES)) == len(ls.ORACLE_CASES + ls.BOTTOMK_CASES)
    for metric in sc.ORACLE_METRICS:
        for method in li.METHODS:
            for n in ls.FULL_NS:
                assert ("dense", metric, method, n) in ls.ORACLE_CASES
    for merges, (n, m) in ls.BORDER.items():
        for method in ("complete", "average"):
            assert ("border", "weightedjaccard", method, n) in ls.ORACLE_CASES


def test_the_chains_end_in_a_tail_at_one_and_the_dense_set_does_not():
    """why the full trees run on a set of their own: the last 65 merges of scale_inputs.chains are at exactly 1.0 under every method"""
    for metric in sc.ORACLE_METRICS:
        d = ls.reference("chains", metric, "single", sc.N)[2]
        assert (d[-65:] == 1.0).all() and d[-66] < 1.0 and sc.N - 1 - ls.C == 64
        D = ls.matrix("dense", metric)
        assert np.nanmax(li.weights_matrix(D)[~np.eye(sc.N, dtype=bool)]) < 1.0, ci.NO_TEST + "a pair of the dense set at 1.0"


@pytest.mark.parametrize("case", ls.ORACLE_CASES, ids=ls.case_id)
def test_the_inputs_are_a_test(case):
    print(ls.case_id(case), ls.check_case(case), "rows rescanned", ls.rows_rescanned(case))


def test_the_cluster_pair_identities_hold_on_the_literal_yardstick():
    """min, max and the mean within 3 roundings a level, at N = 257, on merges no cache produced"""
    for kind, arg, metric in (("random_set", 33, "weightedjaccard"), ("planted_chains", 8, "jaccard"), ("random_set", 8, "jaccard")):
        D = li.named_set(kind, arg, metric)[2]
        for method in li.METHODS:
            used = ls.assert_cluster_pair_identity(D, method, li.reference(kind, arg, metric, method), f"{kind}({arg}) {metric} {method}")
            print(f"{kind}({arg}) {metric} {method}: the largest error is {used:.3f} of its bound")
    # the weighted forest: merges at +inf never happen, so every height is finite; and a wrong height is seen
    D = li.weighted_forest_set()[2]
    for method in li.METHODS:
        ls.assert_cluster_pair_identity(D, method, li.agglomerate(D, method), f"weighted_forest_set {method}")
    D = li.named_set("random_set", 33, "weightedjaccard")[2]
    for method in li.METHODS:
        a, b, d, s = li.reference("random_set", 33, "weightedjaccard", method)
        d = d.copy()
        d[200] = np.nextafter(d[200], 0.0) if method != "average" else d[200] * (1 + 1e-10)
        with pytest.raises(AssertionError):
            ls.assert_cluster_pair_identity(D, method, (a, b, d, s), "a height one step off")
    # depths: a star has depth = its merge number, a balanced tree log2
    lo, hi, mean, depth = ls.cluster_pair_facts(np.full((8, 8), 0.5), [0] * 7, list(range(1, 8)))
    assert depth.tolist() == [1, 2, 3, 4, 5, 6, 7] and (lo == 0.5).all() and (hi == 0.5).all() and (mean == 0.5).all()
    depth = ls.cluster_pair_facts(np.full((8, 8), 0.5), [0, 2, 4, 6, 0, 4, 0], [1, 3, 5, 7, 2, 6, 4])[3]
    assert depth.tolist() == [1, 1, 1, 1, 2, 2, 3]
