"""Single-linkage clustering of a sketch collection on the GPU (hulk_cluster: k_cluster_link, k_cluster_flatten).

The yardstick throughout is oracle.pyorc.smash_matrix over the set plus a plain Python union-find (tests/cluster_inputs.py): edges
where (D <= tau) | (D.T <= tau) off the diagonal, label = the smallest member, links = ((D <= tau) & ~eye).sum().  Labels, clusters
and links are compared exactly.  Every generator's "the inputs are no test" conditions are asserted before anything is compared."""
import os
import subprocess

import numpy as np
import pytest

import cluster_inputs as ci
from conftest import ROOT
from oracle import pyorc

pytestmark = pytest.mark.gpu

METRICS = ("jaccard", "weightedjaccard")


def run(mins, weights, tau, metric, band_rows=0):
    from hulk_amd.smash import cluster
    st = {}
    labels, n_clusters = cluster(mins, weights, tau, metric, band_rows=band_rows, stats=st)
    assert labels.dtype == np.uint32 and labels.shape == (len(mins),) and st["clusters"] == n_clusters
    assert st["bands"] == ci.bands_planned(len(mins), band_rows), (st, band_rows)
    return labels, st["links"], n_clusters


def assert_same(got, want, what):
    gl, gk, gc = got
    wl, wk, wc = want
    bad = np.nonzero(gl != wl)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} labels differ, first at {bad[:5].tolist()}: got {gl[bad[:5]].tolist()}, want {wl[bad[:5]].tolist()}"
    assert (gk, gc) == (wk, wc), f"{what}: links / clusters got {(gk, gc)}, want {(wk, wc)}"


# ---- 1. planted shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 8, 33, 512])
def test_planted_shapes(s):
    """N: one sketch, two, a subject tile of 32 less one, exactly, plus one, a tile of 64 others less one, exactly, plus one, nine
    subject tiles with a tail; S: one slot, less than a chunk of 32, a chunk and a tail, whole chunks.  Every smaller set is the
    first N sketches of the 257 (a pair's distance depends on the pair alone).  The whole product: every N with both metrics and
    every band_rows (N = 33 and 63 in two bands, the second from row 32 on, included)."""
    mins, weights, plan = ci.shapes_plan(s)
    for metric in METRICS:
        D, tau = plan[metric]
        for n in ci.NS:
            want = ci.components(D[:n, :n], tau)
            for band in ci.BANDS:
                assert_same(run(mins[:n], weights[:n], tau, metric, band), want, f"N {n} S {s} {metric} band_rows {band} tau {tau!r}")
        full = ci.components(D, tau)
        print(f"S {s} {metric}: tau {tau!r}, {full[1]} links, {full[2]} clusters at N = 257")


# ---- 2. planted chains ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [8, 33, 512])
def test_planted_chains(s):
    """components held together by chain-neighbour links only, each exactly at tau, with neighbours planted across the tile edges,
    the band edges and the two ends of the set (cluster_inputs.BRIDGES: each is asserted to be a bridge on the yardstick); one ulp
    below tau nothing links"""
    mins, weights, D, members = ci.planted_chains(s)
    tau, want = ci.check_planted_chains(s)
    below = np.nextafter(tau, 0.0)
    for band in ci.BANDS:
        got = run(mins, weights, tau, "jaccard", band)
        assert_same(got, want, f"S {s} band_rows {band}")
        for idx in members:
            assert (got[0][idx] == min(idx)).all()
        got = run(mins, weights, below, "jaccard", band)
        assert got[2] == 257 and got[1] == 0 and np.array_equal(got[0], np.arange(257)), "one ulp below tau: only singletons (the compare is <=, on the double)"


# ---- 3. order stress -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
def test_order_stress(order):
    """one chain of 257: deep parent paths, hooks contended at the same roots, path halving"""
    mins, weights, D = ci.ordered_chain(order)
    tau, want = ci.check_ordered_chain(order)
    for band in ci.BANDS:
        got = run(mins, weights, tau, "jaccard", band)
        assert_same(got, want, f"{order} band_rows {band}")
        assert not got[0].any() and got[2] == 1


# ---- 4. weighted jaccard: one direction is enough ----------------------------------------------------------------------------------
def test_weighted_one_direction_nan_inf_and_the_ends_of_the_range():
    mins, weights, D = ci.weighted_set()
    want = ci.check_weighted_set()
    for tau in (0.5, 0.0, 1.0):
        for band in (0, 32):
            got = run(mins, weights, tau, "weightedjaccard", band)
            assert_same(got, want[tau], f"weighted tau {tau} band_rows {band}")
            labels = got[0]
            if tau == 0.5:
                assert labels[ci.X1] == labels[ci.X0] == ci.X0, "d(X0, X1) <= tau < d(X1, X0): one direction links"
                assert labels[ci.Z] == ci.Y, "an all-zero subject is linked through the other sketch's row"
            if tau == 0.0:
                assert labels[ci.I1] == ci.I0 and labels[ci.Z] == ci.Y
            if tau == 1.0:
                assert got[2] == 1 and not labels.any()
    # the same set under jaccard: the weights (zero, Inf) do not matter
    J = pyorc.smash_matrix(mins, weights, "jaccard")
    for tau in (0.0, 0.5, 1.0):
        assert_same(run(mins, weights, tau, "jaccard", 32), ci.components(J, tau), f"jaccard tau {tau}")


# ---- 5. random sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [8, 33])
def test_random_sets(s):
    mins, weights, per_metric = ci.random_set(s)
    ci.check_random_set(s)
    for metric in METRICS:
        D, taus = per_metric[metric]
        for q, tau in zip((1, 10, 50), taus):
            want = ci.components(D, tau)
            print(f"S {s} {metric} {q} % quantile {tau!r}: {want[1]} links, {want[2]} clusters")
            for band in ci.BANDS:
                assert_same(run(mins, weights, tau, metric, band), want, f"S {s} {metric} tau {tau!r} band_rows {band}")


# ---- 6. invariance -------------------------------------------------------------------------------------------------------------
def test_bands_and_repeats_do_not_change_the_result():
    from hulk_amd.smash import cluster
    mins, weights, per_metric = ci.random_set(33)
    for metric in METRICS:
        tau = per_metric[metric][1][1]
        first = None
        for band, bands in zip(ci.BANDS, (1, 9, 3)):
            for _ in range(2):
                st = {}
                labels, n_clusters = cluster(mins, weights, tau, metric, band_rows=band, stats=st)
                assert st["bands"] == bands
                got = (labels.tobytes(), st["links"], st["clusters"], n_clusters)
                first = first or got
                assert got == first, f"{metric} band_rows {band}"


# ---- 7. the directory form and the CLI ------------------------------------------------------------------------------------------
def write_sketch(path, mins, weights, ksize=21, algo="histosketch"):
    from hulk_amd.sketchio import HULKdata, HistoSketch, KHFSketch, KMVSketch
    d = HULKdata()
    d.filename, d.banner_label = "reads.fq,", "blank"
    if algo == "histosketch":
        d.add(HistoSketch(ksize, np.asarray(mins, dtype=np.uint64), np.asarray(weights, dtype=np.float64), ksize ** 4, False))
    else:
        d.add((KHFSketch if algo == "khf" else KMVSketch)(ksize, len(mins), np.asarray(mins, dtype=np.uint64)))
    d.write_json(path)


def cli(args):
    return subprocess.run(["python", "-m", "hulk_amd"] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)


def render_csv(order, labels):
    from hulk_amd.smash import go_csv_field
    roots = sorted(set(labels.tolist()))
    ordinal = {r: k + 1 for k, r in enumerate(roots)}
    size = np.bincount(labels)
    return "sketch,cluster,size,representative\n" + "".join(
        f"{go_csv_field(p)},{ordinal[int(l)]},{size[l]},{go_csv_field(order[l])}\n" for p, l in zip(order, labels))


def test_directory_form_and_cli(tmp_path):
    """40 sketch files out of the planted chains (one with a comma in its name: encoding/csv quotes it): cluster_files gives the
    array form's labels in sorted path order and writes the CSV a Python rendering gives; the CLI writes the same file and logs the
    counts; --minSimilarity p is --maxDistance 1 - p / 100"""
    from hulk_amd import smash
    s = 8
    all_mins, all_weights, _, members = ci.planted_chains(s)
    pick = members[0][:12] + members[1][:9] + members[2] + members[3][:5] + [i for i in range(257) if not any(i in m for m in members)][:12]
    mins, weights = all_mins[pick], all_weights[pick]
    d = tmp_path / "sk"
    d.mkdir()
    names = [f"s{i:02d}.json" for i in range(40)]
    names[3] = "s,03.json"
    for i, name in enumerate(names):
        write_sketch(str(d / name), mins[i], weights[i])
    order = sorted(str(d / n) for n in names)
    at = [names.index(os.path.basename(p)) for p in order]        # sorted path order -> the arrays' rows
    tau = ci.chain_tau(s)
    for metric, t in (("jaccard", tau), ("weightedjaccard", 0.9)):
        want = smash.cluster(mins[at], weights[at], t, metric)
        D = pyorc.smash_matrix(mins[at], weights[at], metric)
        assert np.array_equal(want[0], ci.components(D, t)[0])
        out = str(tmp_path / f"py_{metric}.csv")
        st = {}
        got_order, labels, n_clusters = smash.cluster_files([str(d / n) for n in names] + [str(d / names[0])], t, metric=metric, csv_path=out, stats=st)
        assert got_order == order and np.array_equal(labels, want[0]) and n_clusters == want[1] == st["clusters"]
        assert st["links"] == ci.components(D, t)[1] and st["bands"] == 1
        text = open(out).read()
        assert text == render_csv(order, labels), text
        assert '"' + str(d / "s,03.json") + '"' in text
        if metric == "jaccard":
            assert 1 < n_clusters < 40 and np.bincount(labels).max() == 12
        r = cli(["cluster", "-d", str(d), "-m", metric, "--maxDistance", repr(t), "-o", str(tmp_path / "cli")])
        assert r.returncode == 0 and "HULK CLUSTER!" in r.stdout, r.stdout + r.stderr
        assert open(str(tmp_path / "cli") + ".hulk-clusters.csv").read() == text
        for line in ("number of sketches: 40", f"number of links: {st['links']}", f"number of clusters: {n_clusters}",
                     f"largest cluster: {int(np.bincount(labels).max())} sketches"):
            assert line in r.stdout, (line, r.stdout)
    # --minSimilarity 75 is --maxDistance 0.25 (S = 8, two fresh slots a step: the chains' own threshold)
    assert tau == 0.25
    a = cli(["cluster", "-d", str(d), "--minSimilarity", "75", "-o", str(tmp_path / "sim")])
    b = cli(["cluster", "-d", str(d), "--maxDistance", "0.25", "-o", str(tmp_path / "dist")])
    assert a.returncode == 0 and b.returncode == 0, a.stdout + b.stdout
    assert open(str(tmp_path / "sim") + ".hulk-clusters.csv").read() == open(str(tmp_path / "dist") + ".hulk-clusters.csv").read() == open(str(tmp_path / "py_jaccard.csv")).read()
    # one file is a set; MinHash signatures carry no weights: jaccard works, weightedjaccard is the reference's refusal
    one_order, one_labels, one_n = smash.cluster_files([str(d / names[0])], 0.5)
    assert one_order == [str(d / names[0])] and one_labels.tolist() == [0] and one_n == 1
    for algo in ("khf", "kmv"):
        m = tmp_path / algo
        m.mkdir()
        for i in range(12):
            write_sketch(str(m / f"m{i:02d}.json"), mins[i], None, algo=algo)
        out = str(tmp_path / f"{algo}.csv")
        got_order, labels, n_clusters = smash.cluster_files([str(p) for p in m.iterdir()], tau, algo=algo, csv_path=out)
        want = ci.components(pyorc.smash_matrix(mins[:12], np.zeros((12, s)), "jaccard"), tau)
        assert np.array_equal(labels, want[0]) and n_clusters == want[2] == 1
        assert open(out).read() == render_csv(got_order, labels)
        r = cli(["cluster", "-d", str(m), "-a", algo, "-m", "weightedjaccard", "--maxDistance", "0.5", "-o", str(tmp_path / algo / "w")])
        assert r.returncode == 1 and "weighted jaccard is only supported for histosketches" in r.stdout


# ---- 8. the C++ host -------------------------------------------------------------------------------------------------------------
def test_cpp_host_matches_the_python_binding(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    exe = str(tmp_path / "cluster_driver")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "cluster_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    s = 33
    mins, weights, per_metric = ci.random_set(s)
    path = str(tmp_path / "sketches.txt")
    with open(path, "w") as fh:
        for a, b in zip(mins, weights):
            fh.write(" ".join([str(int(v)) for v in a] + [float(v).hex() for v in b]) + "\n")
    for metric, band in (("jaccard", 0), ("weightedjaccard", 96), ("jaccard", 32)):
        tau = per_metric[metric][1][0]
        r = subprocess.run([exe, path, str(s), metric, float(tau).hex(), str(band)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        labels, links, n_clusters = run(mins, weights, tau, metric, band)
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 2 and lines[0].split()[0] == "labels"
        assert [int(x) for x in lines[0].split()[1:]] == labels.tolist()
        assert lines[1] == f"stats {links} {ci.bands_planned(257, band)} {n_clusters}"
    r = subprocess.run([exe, path, str(s), "jaccard", "1.5", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("hulk::Error -30|") and "max_distance must be in [0, 1]" in r.stdout


# ---- 9. a search is what it was --------------------------------------------------------------------------------------------------
def test_a_search_before_and_after_a_cluster_call_is_byte_equal():
    from hulk_amd.smash import search
    mins, weights, per_metric = ci.random_set(33)
    for metric in METRICS:
        D, taus = per_metric[metric]
        before = search(mins[:65], weights[:65], mins, weights, 5, metric, "row")
        assert_same(run(mins, weights, taus[1], metric, 32), ci.components(D, taus[1]), metric)
        after = search(mins[:65], weights[:65], mins, weights, 5, metric, "row")
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        # ... and it is the yardstick's: the five closest by (distance, index)
        order = np.lexsort((np.arange(257)[None, :].repeat(65, 0), D[:65]), axis=1)[:, :5]
        ok = ~np.isnan(np.take_along_axis(D[:65], order, 1))
        assert np.array_equal(before[0][ok], order.astype(np.uint32)[ok])
