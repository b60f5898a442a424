"""hulk_linkage past one chunk of LINK_CHUNK = 4096 merges and on forests that end at the chunk's border (tests/linkage_scale_inputs.py):
the merge counter carried across the border, "finished" raised in the last slot of a chunk, in the first slot of the next and one
merge into it, the queued launches behind "finished", more than a chunk of merges copied back, rows_rescanned summed over 261
groups, k_linkage_pick's strided loop in its fifth trip and k_linkage_sym on 131 x 131 tiles with a one-column last tile.

Yardstick: linkage_scale_inputs.agglomerate_cached over the anchored matrix of the set — the oracle's for jaccard and weighted
jaccard (the GPU's distance_matrix equals it: every number in every bit, NaN where it has NaN), the GPU's own for bottomk, held to
bottomk_inputs.matrix on a 64-sketch sample.  tests/test_linkage_scale_cpu.py holds agglomerate_cached to the literal argmin of
linkage_inputs.agglomerate.  One run of it at N = 4161 takes 0.7 - 1.9 s on one x86 core (measured per case; complete
linkage under weighted jaccard on the dense set is the slowest, most cases are at 0.8 - 1.0 s), the O(N^2) cluster-pair identities
0.45 s, so a case is 2 - 3 s with its two GPU calls (about 1 s on the GPU machine's host) and no case was dropped.  Every "the inputs
are no test" condition is asserted before anything is compared."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bottomk_inputs as bi
import dendrogram_inputs as di
import linkage_inputs as li
import linkage_scale_inputs as ls
import scale_inputs as sc
from conftest import ROOT
from test_gpu_collection_scale import yardstick as scale_yardstick
from test_gpu_linkage import assert_same, run

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def anchor(name, metric):
    """the matrix a set's cases are prefixes of, anchored on the GPU's distance_matrix"""
    if name in sc.SETS:
        return scale_yardstick(name, metric)
    from hulk_amd.smash import distance_matrix
    mins, weights = ls.arrays(name)
    G = distance_matrix(mins, None if metric == "bottomk" else weights, metric)
    assert G.shape == (ls.N, ls.N) and G.dtype == np.float64
    if metric in sc.ORACLE_METRICS:
        D = ls.matrix(name, metric)
        nan = np.isnan(D)
        bad = np.argwhere((np.isnan(G) != nan) | (~nan & (di.bits(G) != di.bits(D))))
        assert len(bad) == 0, f"{name} {metric}: {len(bad)} entries differ from the oracle's, first at {bad[:3].tolist()}"
        return D
    idx = np.sort(np.random.default_rng(9700).permutation(ls.N)[:sc.SAMPLE])
    want = bi.matrix(mins[idx])
    assert np.array_equal(di.bits(G[np.ix_(idx, idx)]), di.bits(want)), f"{name} bottomk: the sampled sub-matrix differs from the yardstick's"
    assert np.array_equal(di.bits(G), di.bits(G.T)) and not np.diag(G).any() and not np.isnan(G).any()
    return sc.give_matrix(name, metric, G)


# ---- 1. the anchors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["border", "inside"])
def test_forest_matrix_anchor(name):
    """the all-zero weight rows are NaN as subjects, everybody else's row reaches them"""
    ls.check_sizes()
    D = anchor(name, "weightedjaccard")
    z = ls.zeroed(name)
    rest = np.setdiff1d(np.arange(ls.N), z)
    assert np.isnan(D[z]).all() and not np.isnan(D[rest]).any()
    print(f"{name}: {len(z)} rows of NaN")


@pytest.mark.parametrize("metric", sc.METRICS)
def test_dense_matrix_anchor(metric):
    D = anchor("dense", metric)
    off = D[~np.eye(ls.N, dtype=bool)]
    assert off.max() < 1.0, li.NO_TEST + "a pair of the dense set at 1.0"
    print(f"dense {metric}: distances {off.min()!r} .. {off.max()!r}, {len(np.unique(off))} distinct")


# ---- 2. every case against the yardstick ---------------------------------------------------------------------------------------------
def run_case(case):
    name, metric, method, n = case
    D = anchor(name, metric)
    ls.check_sizes()
    facts = ls.check_case(case)                                 # (before anything is compared)
    want = ls.reference(*case)
    mins, weights = ls.arrays(name)
    mins, weights = mins[:n], (None if metric == "bottomk" else weights[:n])
    got, st = run(mins, weights, method, metric)
    what = ls.case_id(case)
    print(f"{what}: {facts}; {st['merges']} merges, {st['components']} clusters left, {st['rows_rescanned']} rows rescanned, merges "
          f"{st['kernel_ms_merge']:.1f} ms")
    assert_same(got, want, what)
    assert st["merges"] == ls.wanted_merges(case) == len(want[0]) and st["components"] == n - st["merges"], (what, st)
    assert st["rows_rescanned"] >= n + st["merges"], (what, st)
    assert st["rows_rescanned"] == ls.rows_rescanned(case), f"{what}: {st['rows_rescanned']} rows rescanned, the same rule on the host scans {ls.rows_rescanned(case)}"
    again, st2 = run(mins, weights, method, metric)
    assert [x.tobytes() for x in again] == [x.tobytes() for x in got], f"{what}: a second call differs"
    assert (st2["merges"], st2["components"], st2["rows_rescanned"]) == (st["merges"], st["components"], st["rows_rescanned"]), (what, st, st2)
    # what needs no yardstick of the merge order: every pair lies across exactly one merge
    used = ls.assert_cluster_pair_identity(D[:n, :n], method, got, what)
    if method == "average":
        print(f"{what}: the largest error against the mean is {used:.3f} of its bound")
    if name in ("border", "inside") and method != "single":
        z = ls.zeroed(name)
        z = z[z < n]
        held = [len(np.intersect1d(np.array(sorted(m)), z)) for m in li.member_sets(n, got[0], got[1])]
        assert max(held) == 1, f"{what}: a cluster holds {max(held)} zeroed sketches"
    return got, st


@pytest.mark.parametrize("case", ls.FOREST_CASES, ids=ls.case_id)
def test_forests_that_end_at_the_chunk_border(case):
    """weighted jaccard with all-zero weight rows: C - 1, C and C + 1 merges at N > C — "finished" is raised by the pick in the last
    slot of chunk one (no second chunk may be queued: the loop's own bound stops it, the state is read once), in the first slot of
    chunk two and in its second; 300 merges at N = 4161 with 3 * 3,796 launches queued behind "finished"; and single linkage on that
    set, which is one tree"""
    got, st = run_case(case)
    if case[2] == "single":
        assert st["merges"] == case[3] - 1 and st["components"] == 1


@pytest.mark.parametrize("case", ls.FULL_BORDER_CASES, ids=ls.case_id)
def test_full_trees_round_the_chunk_border(case):
    """N - 1 = C - 1, C and C + 1: the loop ends inside the first chunk, exactly at its end, and one merge into the second"""
    run_case(case)


@pytest.mark.parametrize("case", ls.WHOLE_CASES, ids=ls.case_id)
def test_full_trees_of_the_whole_sets(case):
    """N = 4161: 64 merges in chunk two — below 1.0 on the dense set, the tail at 1.0 on the chains; far_pairs: merges whose p
    k_linkage_pick reads in the fifth trip of its loop"""
    got, st = run_case(case)
    if case[2] != "average":
        assert (np.diff(got[2]) >= 0).all(), "heights never step down"


@pytest.mark.parametrize("case", ls.BOTTOMK_CASES, ids=ls.case_id)
def test_bottomk_complete(case):
    run_case(case)


# ---- 3. single linkage is the dendrogram and the clustering ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", sc.ORACLE_METRICS)
def test_single_linkage_is_the_spanning_forest_and_every_cut_the_clustering(metric):
    from hulk_amd.smash import cluster, cut_dendrogram, dendrogram
    anchor("chains", metric)
    sc.check_chains("chains", metric)
    mins, weights = ls.arrays("chains")
    (a, b, d, size), st = run(mins, weights, "single", metric)
    assert st["merges"] == ls.N - 1 > ls.C
    ea, eb, ed = dendrogram(mins, weights, metric)
    assert np.array_equal(np.sort(li.bits(d)), np.sort(li.bits(ed))), "the heights are hulk_dendrogram's edge distances as a multiset of bits"
    assert np.array_equal(np.sort(li.bits(d)), np.sort(li.bits(sc.forest("chains", metric)[2])))
    taus = sc.thresholds("chains", metric)
    assert taus[0] == sc.TAU
    for tau in taus:
        labels, k = cut_dendrogram(ls.N, a, b, d, tau)
        want = cluster(mins, weights, tau, metric)
        assert np.array_equal(labels, want[0]) and k == want[1], (metric, tau)
        assert np.array_equal(labels, sc.clustering("chains", metric, tau)[0]) and 1 < k < ls.N


# ---- 4. the C++ host ---------------------------------------------------------------------------------------------------------------------
def test_cpp_host_past_one_chunk(tmp_path):
    """tests/cpp/linkage_driver.cpp takes any number of sketches through its file: the border forest of exactly C merges and the
    whole dense set, against the Python binding"""
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    exe = str(tmp_path / "linkage_driver")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "linkage_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    for case in (("border", "weightedjaccard", "complete", ls.BORDER[ls.C][0]), ("dense", "jaccard", "average", ls.N)):
        name, metric, method, n = case
        mins, weights = ls.arrays(name)
        path = str(tmp_path / f"{name}.txt")
        with open(path, "w") as fh:
            for m, w in zip(mins[:n], weights[:n]):
                fh.write(" ".join([str(int(v)) for v in m] + [float(v).hex() for v in w]) + "\n")
        r = subprocess.run([exe, path, str(ls.S), metric, method], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        (a, b, d, size), st = run(mins[:n], weights[:n], method, metric)
        assert st["merges"] == ls.wanted_merges(case) >= ls.C
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(a) + 1
        got = [line.split() for line in lines[:-1]]
        assert all(g[0] == "merge" for g in got)
        assert [int(g[1]) for g in got] == a.tolist() and [int(g[2]) for g in got] == b.tolist() and [int(g[4]) for g in got] == size.tolist()
        assert [float.fromhex(g[3]) for g in got] == d.tolist()
        assert lines[-1] == f"stats {st['merges']} {st['components']} {st['rows_rescanned']}"
