"""The links of a sketch collection as a sparse graph on the GPU (hulk_links: k_links_count, k_links_rows, k_links_scan, k_links_fill).

The yardstick throughout is tests/links_inputs.py: from oracle.pyorc.smash_matrix's D (tests/bottomk_inputs.py's for the bottom-k
metric), row i is np.flatnonzero((D[i] <= tau) & (arange != i)) and its distances are D[i, those].  indptr, indices and the distance
BITS are compared for equality.  Every input's "the inputs are no test" conditions are asserted before anything is compared."""
import functools
import os
import subprocess

import numpy as np
import pytest

import bottomk_inputs as bi
import cluster_inputs as ci
import links_inputs as li
from conftest import ROOT
from oracle import pyorc
from test_gpu_cluster import cli, write_sketch

pytestmark = pytest.mark.gpu

METRICS = li.METRICS


def run(mins, weights, tau, metric, band_rows=0, upper=False, max_edges=0):
    from hulk_amd.smash import links
    st = {}
    got = links(mins, weights, tau, metric, upper=upper, max_edges=max_edges, band_rows=band_rows, stats=st)
    n = len(mins)
    assert got[0].shape == (n + 1,) and got[1].shape == got[2].shape == (int(got[0][-1]),) and got[0][0] == 0
    assert st["edges"] == int(got[0][-1]) and st["bands"] == ci.bands_planned(n, band_rows), (st, band_rows)
    assert st["max_degree"] == (int(li.degrees(got[0]).max()) if n else 0), st
    return got


# ---- 1. planted chains ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [8, 33, 512])
def test_planted_chains(s):
    """the links are the chain neighbours, each exactly at tau, on the tile edges and the band edges by construction; one ulp below
    tau jaccard lists nothing (the compare is <=, on the double)"""
    mins, weights, D, members = ci.planted_chains(s)
    tau = li.check_chain_links(s)
    below = np.nextafter(tau, 0.0)
    for metric in METRICS:
        want, want_below = li.csr(D[metric], tau), li.csr(D[metric], below)
        for band in ci.BANDS:
            li.assert_same(run(mins, weights, tau, metric, band), want, f"S {s} {metric} band_rows {band}")
            got = run(mins, weights, below, metric, band)
            li.assert_same(got, want_below, f"S {s} {metric} band_rows {band}, one ulp below")
            if metric == "jaccard":
                assert int(got[0][-1]) == 0 and not got[0].any()
    assert int(li.csr(D["jaccard"], tau)[0][-1]) == 2 * sum(len(m) - 1 for m in members)


# ---- 2. weighted jaccard is directed ----------------------------------------------------------------------------------------------
def test_weighted_one_direction_nan_inf_and_the_ends_of_the_range():
    mins, weights, D = ci.weighted_set()
    wants = li.check_weighted_links()
    for tau in (0.0, 0.5, 1.0):
        for band in (0, 32):
            got = run(mins, weights, tau, "weightedjaccard", band)
            li.assert_same(got, wants[tau], f"weighted tau {tau} band_rows {band}")
            ptr, idx, dist = got
            row = lambda i: idx[int(ptr[i]):int(ptr[i + 1])].tolist()
            assert row(ci.Z) == [], "a NaN subject has an empty row"
            if tau == 0.5:
                assert ci.X1 in row(ci.X0) and ci.X0 not in row(ci.X1), "d(X0, X1) <= tau < d(X1, X0): in X0's row only"
                assert ci.Z in row(ci.Y), "... and still appears in Y's row"
            if tau == 0.0:
                assert ci.I1 in row(ci.I0) and ci.I0 in row(ci.I1) and ci.Z in row(ci.Y) and not dist.any()
            if tau == 1.0:
                assert ci.V not in row(ci.U) and ci.I0 in row(ci.U), "the Inf weight: NaN where the slot is shared, 1.0 elsewhere"
    # the same set under jaccard: the weights (zero, Inf) do not matter
    J = pyorc.smash_matrix(mins, weights, "jaccard")
    for tau in (0.0, 0.5, 1.0):
        li.assert_same(run(mins, weights, tau, "jaccard", 32), li.csr(J, tau), f"jaccard tau {tau}")


# ---- 3. random sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 8, 33])
def test_random_sets(s):
    mins, weights, per_metric = ci.random_set(s)
    li.check_random_links(s)
    for metric in METRICS:
        D, taus = per_metric[metric]
        for tau in list(taus) + [1.0]:
            want = li.csr(D, tau)
            print(f"S {s} {metric} tau {tau!r}: {int(want[0][-1])} edges, largest degree {int(li.degrees(want[0]).max())}")
            for band in ci.BANDS:
                st_got = run(mins, weights, tau, metric, band)
                li.assert_same(st_got, want, f"S {s} {metric} tau {tau!r} band_rows {band}")
        full = run(mins, weights, 1.0, metric)
        assert int(full[0][-1]) == int((~np.isnan(D) & ~np.eye(257, dtype=bool)).sum())
        if metric == "jaccard":
            assert int(li.degrees(full[0]).max()) == 256


# ---- 4. small N ----------------------------------------------------------------------------------------------------------------
def test_small_n():
    """N: one sketch, two, a subject tile of 32 less one, exactly, plus one, a tile of 64 others less one, exactly, plus one, nine
    subject tiles with a tail — as prefixes of one set (a pair's distance depends on the pair alone)"""
    mins, weights, per_metric = ci.random_set(33)
    for metric in METRICS:
        D, taus = per_metric[metric]
        for n in ci.NS:
            for tau in (taus[1], 1.0):
                want = li.csr(D[:n, :n], tau)
                for band in ci.BANDS:
                    li.assert_same(run(mins[:n], weights[:n], tau, metric, band), want, f"N {n} {metric} tau {tau!r} band_rows {band}")
    one = run(mins[:1], weights[:1], 1.0, "jaccard")
    assert one[0].tolist() == [0, 0] and len(one[1]) == 0 and len(one[2]) == 0


# ---- 5. more than one default band -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_set():
    n, s = 2113, 8
    rng = np.random.default_rng(7400)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    keep = rng.random((n, s)) < (0.2 + 0.6 * rng.random((n, 1)))
    mins = np.where(keep, base, rng.integers(0, 194481, size=(n, s)).astype(np.uint64))
    mins[n - 1] = mins[5]                                           # the one column of the last tile is linked from the first band
    mins[2048] = mins[2047]                                         # ... and the last row of the first band to the first of the second
    weights = -rng.gamma(2.0, 1e-3, size=(n, s))
    mins.setflags(write=False); weights.setflags(write=False)
    return mins, weights


def test_more_than_one_default_band():
    """N = 2113: band_rows = 0 gives one band of 2048 rows and one of 65, and the last column tile holds one column.  Against the
    thresholded distance matrix of the GPU, at a distance that occurs near the 0.1 % quantile"""
    from hulk_amd.smash import distance_matrix
    mins, weights = big_set()
    n = len(mins)
    D = distance_matrix(mins, weights, "jaccard")
    off = D[~np.eye(n, dtype=bool)]
    tau = float(np.quantile(off, 0.001, method="lower"))
    want = li.csr(D, tau)
    e = int(want[0][-1])
    assert 0 < e < n * (n - 1) // 4 and 0 <= tau < 1, li.NO_TEST + f"tau {tau!r}: {e} edges"
    assert int(want[0][2048]) not in (0, e) and (want[1] == n - 1).any(), li.NO_TEST + "edges in both bands, and in the last column"
    assert D[5, n - 1] == 0 == D[n - 1, 5] and D[2047, 2048] == 0 == D[2048, 2047], li.NO_TEST + "the planted pairs"
    from hulk_amd.smash import links
    st = {}
    got = links(mins, weights, tau, "jaccard", stats=st)
    assert st["bands"] == 2 and st["edges"] == e
    li.assert_same(got, want, f"N {n} tau {tau!r}")
    print(f"N {n}: tau {tau!r}, {e} edges, largest degree {st['max_degree']}")
    li.assert_same(links(mins, weights, tau, "jaccard", upper=True), li.csr(D, tau, upper=True), f"N {n} upper")


# ---- 6. the upper flag ----------------------------------------------------------------------------------------------------------
def test_upper_is_the_full_result_filtered():
    mins, weights, per_metric = ci.random_set(33)
    for metric in METRICS:
        D, taus = per_metric[metric]
        for tau in (taus[1], 1.0):
            full = run(mins, weights, tau, metric, 32)
            for band in ci.BANDS:
                up = run(mins, weights, tau, metric, band, upper=True)
                li.assert_same(up, li.upper_of(*full), f"{metric} tau {tau!r} band_rows {band}")
                li.assert_same(up, li.csr(D, tau, upper=True), f"{metric} tau {tau!r} band_rows {band} (yardstick)")
            if metric == "jaccard":
                assert 2 * int(up[0][-1]) == int(full[0][-1]), "symmetric: the graph without its mirror image"
    m, D = bottomk_collection()
    tau = bottomk_taus(D)[1]
    full = run(m, None, tau, "bottomk", 32)
    up = run(m, None, tau, "bottomk", 32, upper=True)
    li.assert_same(up, li.upper_of(*full), "bottomk upper")
    assert 2 * int(up[0][-1]) == int(full[0][-1]) > 0


# ---- 7. bottom-k ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bottomk_collection():
    m = bi.random_set(130, 50, 180, spread=2)
    D = bi.matrix(m)
    m.setflags(write=False); D.setflags(write=False)
    return m, D


def bottomk_taus(D):
    off = np.unique(D[~np.eye(len(D), dtype=bool)])
    return [float(off[len(off) // 8]), float(off[len(off) // 4]), 1.0]


def test_bottomk():
    """weights NULL; thresholds that are distances of the set (equality is in), the planted lists of the metric's own tests"""
    m, D = bottomk_collection()
    for tau in bottomk_taus(D):
        want = li.csr(D, tau)
        assert int(want[0][-1]) > 0
        for band in ci.BANDS:
            li.assert_same(run(m, None, tau, "bottomk", band), want, f"bottomk tau {tau!r} band_rows {band}")
    for n, s in ((97, 33), (65, 512)):
        p = bi.planted_set(n, s)
        P = bi.matrix(p)
        for tau in (0.0, 0.5, 1.0):
            li.assert_same(run(p, None, tau, "bottomk", 32), li.csr(P, tau), f"bottomk planted N {n} S {s} tau {tau}")


# ---- 8. cross-checks on the GPU ---------------------------------------------------------------------------------------------------
def test_cluster_and_the_matrix_agree_with_the_list():
    from hulk_amd.smash import cluster, distance_matrix
    mins, weights, per_metric = ci.random_set(33)
    sets = [(mins, weights, metric, per_metric[metric][1][0]) for metric in METRICS]
    m, D = bottomk_collection()
    sets.append((m, None, "bottomk", bottomk_taus(D)[0]))
    for a, w, metric, tau in sets:
        n = len(a)
        ptr, idx, dist = run(a, w, tau, metric, 32)
        st = {}
        labels, n_clusters = cluster(a, w, tau, metric, stats=st)
        assert int(ptr[-1]) == st["links"] > 0, metric
        rows = np.repeat(np.arange(n), li.degrees(ptr))
        assert np.array_equal(ci.union_find_labels(n, zip(rows.tolist(), idx.tolist())), labels), f"{metric}: a union-find over the listed edges gives cluster's labels"
        assert 1 < n_clusters < n
        G = distance_matrix(a, w, metric)
        assert np.array_equal(dist.view(np.uint64), G[rows, idx].view(np.uint64)), f"{metric}: a listed distance is the matrix entry, bit for bit"


# ---- 9. repeats --------------------------------------------------------------------------------------------------------------
def test_bands_and_repeats_do_not_change_a_byte():
    mins, weights, per_metric = ci.random_set(33)
    for metric in METRICS:
        tau = per_metric[metric][1][1]
        for upper in (False, True):
            first = None
            for band in (32, 96, 0):
                for _ in range(2):
                    got = tuple(x.tobytes() for x in run(mins, weights, tau, metric, band, upper=upper))
                    first = first or got
                    assert got == first, f"{metric} band_rows {band} upper {upper}"


# ---- 10. the cap ---------------------------------------------------------------------------------------------------------------
def test_max_edges():
    from hulk_amd._lib import HulkError
    from hulk_amd.smash import links
    mins, weights, per_metric = ci.random_set(33)
    D, taus = per_metric["jaccard"]
    want = li.csr(D, taus[1])
    e = int(want[0][-1])
    assert e > 1
    li.assert_same(run(mins, weights, taus[1], "jaccard", 32, max_edges=e), want, "max_edges = the count")
    li.assert_same(run(mins, weights, taus[1], "jaccard", 0, max_edges=e), want, "max_edges = the count, one band")
    last_row = int(np.flatnonzero(li.degrees(want[0]))[-1])
    for band in (0, 32):
        st = {}
        with pytest.raises(HulkError) as ei:
            links(mins, weights, taus[1], "jaccard", max_edges=e - 1, band_rows=band, stats=st)
        assert ei.value.code == -30 and f"max_edges = {e - 1}" in ei.value.message, ei.value.message
        # one below the count: the cap is crossed in the band of the last edge, with every edge counted
        assert st["edges"] == e and f"edges: {e} " in ei.value.message, (st, ei.value.message)
        assert st["bands"] == (last_row // band + 1 if band else 1), st
    # a cap in the first band of several: the later bands are not counted
    st = {}
    with pytest.raises(HulkError):
        links(mins, weights, 1.0, "jaccard", max_edges=100, band_rows=32, stats=st)
    assert st["bands"] == 1 and st["edges"] == 32 * 256


# ---- 11. the directory form and the CLI ------------------------------------------------------------------------------------------
def test_directory_form_and_cli(tmp_path):
    """40 sketch files out of the planted chains (one with a comma in its name: encoding/csv quotes it): links_files gives the array
    form's result in sorted path order and writes the CSV a Python rendering of the yardstick gives; the CLI writes the same file
    and logs the counts; --minSimilarity p is --maxDistance 1 - p / 100"""
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
    for metric, t, upper in (("jaccard", tau, False), ("weightedjaccard", 0.9, False), ("jaccard", tau, True)):
        D = pyorc.smash_matrix(mins[at], weights[at], metric)
        want = li.csr(D, t, upper=upper)
        assert int(want[0][-1]) > 0
        out = str(tmp_path / f"py_{metric}_{int(upper)}.csv")
        st = {}
        got = smash.links_files([str(d / n) for n in names] + [str(d / names[0])], t, metric=metric, upper=upper, csv_path=out, stats=st)
        assert got[0] == order
        li.assert_same(got[1:], want, f"links_files {metric} upper {upper}")
        li.assert_same(smash.links(mins[at], weights[at], t, metric, upper=upper), want, f"links {metric} upper {upper}")
        assert st["edges"] == int(want[0][-1]) and st["bands"] == 1 and st["max_degree"] == int(li.degrees(want[0]).max())
        text = open(out).read()
        assert text == li.render_csv(order, want), text
        assert '"' + str(d / "s,03.json") + '"' in text
        r = cli(["links", "-d", str(d), "-m", metric, "--maxDistance", repr(t), "-o", str(tmp_path / "cli")] + (["--upper"] if upper else []))
        assert r.returncode == 0 and "HULK LINKS!" in r.stdout, r.stdout + r.stderr
        assert open(str(tmp_path / "cli") + ".hulk-links.csv").read() == text
        for line in ("number of sketches: 40", f"number of edges: {st['edges']}", f"largest degree: {st['max_degree']}", "bands: 1"):
            assert line in r.stdout, (line, r.stdout)
    # --minSimilarity 75 is --maxDistance 0.25 (S = 8, two fresh slots a step: the chains' own threshold)
    assert tau == 0.25
    a = cli(["links", "-d", str(d), "--minSimilarity", "75", "-o", str(tmp_path / "sim")])
    b = cli(["links", "-d", str(d), "--maxDistance", "0.25", "-o", str(tmp_path / "dist")])
    assert a.returncode == 0 and b.returncode == 0, a.stdout + b.stdout
    assert open(str(tmp_path / "sim") + ".hulk-links.csv").read() == open(str(tmp_path / "dist") + ".hulk-links.csv").read() == open(str(tmp_path / "py_jaccard_0.csv")).read()
    # the cap through the CLI: exit code 1, the text
    c = cli(["links", "-d", str(d), "--maxDistance", "0.25", "--maxEdges", "3", "-o", str(tmp_path / "cap")])
    assert c.returncode == 1 and "max_edges = 3" in c.stdout, c.stdout
    # one file is a set; MinHash signatures carry no weights: jaccard works, weightedjaccard is the reference's refusal
    one = smash.links_files([str(d / names[0])], 0.5, csv_path=str(tmp_path / "one.csv"))
    assert one[0] == [str(d / names[0])] and one[1].tolist() == [0, 0] and len(one[2]) == 0 and len(one[3]) == 0
    assert open(str(tmp_path / "one.csv")).read() == "sketch,neighbour,distance,similarity\n"
    for algo in ("khf", "kmv"):
        m = tmp_path / algo
        m.mkdir()
        for i in range(12):
            write_sketch(str(m / f"m{i:02d}.json"), mins[i], None, algo=algo)
        out = str(tmp_path / f"{algo}.csv")
        got = smash.links_files([str(p) for p in m.iterdir()], tau, algo=algo, csv_path=out)
        want = li.csr(pyorc.smash_matrix(mins[:12], np.zeros((12, s)), "jaccard"), tau)
        li.assert_same(got[1:], want, algo)
        assert open(out).read() == li.render_csv(got[0], want)
        r = cli(["links", "-d", str(m), "-a", algo, "-m", "weightedjaccard", "--maxDistance", "0.5", "-o", str(tmp_path / algo / "w")])
        assert r.returncode == 1 and "weighted jaccard is only supported for histosketches" in r.stdout
    got = smash.links_files([str(p) for p in (tmp_path / "kmv").iterdir()], 0.5, algo="kmv", metric="bottomk")
    li.assert_same(got[1:], li.csr(bi.matrix(mins[:12]), 0.5), "bottomk files")


# ---- 12. the C++ host ------------------------------------------------------------------------------------------------------------
def test_cpp_host_matches_the_python_binding(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    exe = str(tmp_path / "links_driver")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "links_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    s = 33
    mins, weights, per_metric = ci.random_set(s)
    path = str(tmp_path / "sketches.txt")
    with open(path, "w") as fh:
        for a, b in zip(mins, weights):
            fh.write(" ".join([str(int(v)) for v in a] + [float(v).hex() for v in b]) + "\n")
    for metric, band, upper in (("jaccard", 0, False), ("weightedjaccard", 96, False), ("jaccard", 32, True)):
        tau = per_metric[metric][1][0]
        r = subprocess.run([exe, path, str(s), metric, float(tau).hex(), str(int(upper)), "0", str(band)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        ptr, idx, dist = run(mins, weights, tau, metric, band, upper=upper)
        lines = r.stdout.strip().splitlines()
        assert [l.split()[0] for l in lines] == ["indptr", "indices", "distances", "stats"]
        assert [int(x) for x in lines[0].split()[1:]] == ptr.tolist()
        assert [int(x) for x in lines[1].split()[1:]] == idx.tolist()
        assert [int(x, 16) for x in lines[2].split()[1:]] == dist.view(np.uint64).tolist()
        assert lines[3] == f"stats {int(ptr[-1])} {ci.bands_planned(257, band)} {int(li.degrees(ptr).max())}"
    r = subprocess.run([exe, path, str(s), "jaccard", "1.5", "0", "0", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("hulk::Error -30|") and "max_distance must be in [0, 1]" in r.stdout
    r = subprocess.run([exe, path, str(s), "jaccard", "1.0", "0", "5", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("hulk::Error -30|") and "max_edges = 5" in r.stdout


# ---- 13. a clustering is what it was ----------------------------------------------------------------------------------------------
def test_a_cluster_call_before_and_after_a_links_call_is_the_same():
    from hulk_amd.smash import cluster
    mins, weights, per_metric = ci.random_set(33)
    for metric in METRICS:
        D, taus = per_metric[metric]
        st0, st1 = {}, {}
        before = cluster(mins, weights, taus[1], metric, band_rows=32, stats=st0)
        li.assert_same(run(mins, weights, taus[1], metric, 32), li.csr(D, taus[1]), metric)
        after = cluster(mins, weights, taus[1], metric, band_rows=32, stats=st1)
        assert np.array_equal(before[0], after[0]) and before[1] == after[1] and st0["links"] == st1["links"]
        want = ci.components(D, taus[1])
        assert np.array_equal(before[0], want[0]) and st0["links"] == want[1]
