"""The single-linkage dendrogram of a sketch collection on the GPU (hulk_dendrogram: k_dendro_offer, k_dendro_fold, the host
contraction of hulk_boruvka.h).

The yardstick throughout is tests/dendrogram_inputs.py: oracle.pyorc.smash_matrix over the set, W = fmin(D, D.T), Kruskal over the
non-NaN pairs sorted by (W, i, j).  Index arrays are compared as equal and distances as bits; the "the inputs are no test"
conditions of every generator are asserted before anything is compared."""
import os
import subprocess

import numpy as np
import pytest

import cluster_inputs as ci
import dendrogram_inputs as di
from conftest import ROOT
from oracle import pyorc

pytestmark = pytest.mark.gpu


def run(mins, weights, metric, band_rows=0):
    from hulk_amd.smash import dendrogram
    st = {}
    a, b, d = dendrogram(mins, weights, metric, band_rows=band_rows, stats=st)
    n = len(mins)
    assert a.dtype == np.uint32 and b.dtype == np.uint32 and d.dtype == np.float64 and len(a) == len(b) == len(d) == st["edges"]
    assert st["components"] == n - len(a) and st["bands"] == ci.bands_planned(n, band_rows), (st, band_rows)
    assert st["rounds"] <= di.round_bound(n), st
    assert (a < b).all() and (b < n).all()
    return (a, b, d), st


def assert_same(got, want, what):
    ga, gb, gd = got
    wa, wb, wd = want
    assert len(ga) == len(wa), f"{what}: {len(ga)} edges, want {len(wa)}"
    bad = np.nonzero((ga != wa) | (gb != wb) | (di.bits(gd) != di.bits(wd)))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} edges differ, first at {bad[:3].tolist()}: got "
                           f"{[(int(ga[i]), int(gb[i]), float(gd[i]).hex()) for i in bad[:3]]}, want {[(int(wa[i]), int(wb[i]), float(wd[i]).hex()) for i in bad[:3]]}")


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 8, 33, 512])
def test_shapes(s):
    """N: one sketch, two, a subject tile of 32 less one, exactly, plus one, a tile of 64 others less one, exactly, plus one, nine
    subject tiles with a tail (the padded rows behind N agree in every slot: unmasked they would win every minimum); S: one slot,
    less than a chunk of 32, a chunk and a tail, whole chunks.  Every smaller set is the first N sketches of the 257.  The whole
    product with both metrics and every band_rows."""
    kind, arg = di.shapes_set(s)
    for metric in di.METRICS:
        mins, weights, D = di.named_set(kind, arg, metric)
        for n in ci.NS:
            want = di.reference(kind, arg, metric, n)
            for band in ci.BANDS:
                got, st = run(mins[:n], weights[:n], metric, band)
                assert_same(got, want, f"N {n} S {s} {metric} band_rows {band}")
                if n == 1:
                    assert st["rounds"] == 0 and st["edges"] == 0 and st["components"] == 1
        print(f"S {s} {metric}: {len(want[0])} edges at N = 257, heights {want[2][0]!r} .. {want[2][-1]!r}")


# ---- 2. many rounds: the filter comp[s] != comp[q] ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(di.MULTI_ROUND)))
def test_many_rounds(which):
    """sets on which the offer form needs 4 - 5 rounds: the result is exact and the number of rounds the yardstick's, which is
    deterministic because every component picks in every round"""
    kind, arg, metric = di.MULTI_ROUND[which]
    want_rounds = di.check_multi_round()[(kind, arg, metric)]
    mins, weights, D = di.named_set(kind, arg, metric)
    for band in ci.BANDS:
        got, st = run(mins, weights, metric, band)
        assert_same(got, di.reference(kind, arg, metric), f"{kind}({arg}) {metric} band_rows {band}")
        assert st["rounds"] == want_rounds, (st, want_rounds)


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_ordered_chains(order):
    mins, weights, D = ci.ordered_chain(order)
    ci.check_ordered_chain(order)
    want_rounds = di.reference_rounds("ordered_chain", order, "jaccard")
    for band in ci.BANDS:
        got, st = run(mins, weights, "jaccard", band)
        assert_same(got, di.reference("ordered_chain", order, "jaccard"), f"{order} band_rows {band}")
        assert st["rounds"] == want_rounds


@pytest.mark.parametrize("s", [8, 33])
def test_random_sets(s):
    ci.check_random_set(s)
    for metric in di.METRICS:
        mins, weights, D = di.named_set("random_set", s, metric)
        want_rounds = di.reference_rounds("random_set", s, metric)
        for band in ci.BANDS:
            got, st = run(mins, weights, metric, band)
            assert_same(got, di.reference("random_set", s, metric), f"S {s} {metric} band_rows {band}")
            assert st["rounds"] == want_rounds


# ---- 3. directions, NaN, Inf -----------------------------------------------------------------------------------------------------------
def test_weighted_directions_nan_and_inf():
    mins, weights, D = ci.weighted_set()
    at = di.check_weighted_facts()
    want = di.reference("weighted_set", None, "weightedjaccard")
    for band in (0, 32):
        got, st = run(mins, weights, "weightedjaccard", band)
        assert_same(got, want, f"weighted band_rows {band}")
        edges = {(int(x), int(y)): h for x, y, h in zip(*got)}
        assert di.bits(edges[(ci.X0, ci.X1)]) == di.bits(D[ci.X0, ci.X1]) != di.bits(D[ci.X1, ci.X0]), "the smaller direction's bits"
        assert edges[(ci.Y, ci.Z)] == 0 and [e for e in edges if ci.Z in e] == [(ci.Y, ci.Z)], "an all-zero subject hangs on the other sketch's row"
        assert di.bits(edges[(ci.U, ci.V)]) == di.bits(D[ci.V, ci.U]) and np.isnan(D[ci.U, ci.V]), "a NaN direction is ignored"
        assert edges[(ci.I0, ci.I1)] == 0
        assert st["edges"] == 64 and st["components"] == 1
    # the same set under jaccard: the weights (zero, Inf) do not matter
    for band in (0, 32):
        got, st = run(mins, weights, "jaccard", band)
        assert_same(got, di.reference("weighted_set", None, "jaccard"), f"jaccard band_rows {band}")


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------------------
def test_ties_stars_and_a_set_without_any_edge():
    for (mins, weights), h in ((di.identical_set(), 0.0), (di.disjoint_set(), 1.0)):
        for metric in di.METRICS:
            for band in (0, 32):
                (a, b, d), st = run(mins, weights, metric, band)
                assert not a.any() and b.tolist() == list(range(1, 65)) and (di.bits(d) == di.bits(np.full(64, h))).all(), (metric, band, h)
                assert st["rounds"] == 1 and st["components"] == 1
    mins, weights = di.zero_weight_set()
    (a, b, d), st = run(mins, weights, "weightedjaccard")
    assert len(a) == 0 and st["edges"] == 0 and st["components"] == 3 and st["rounds"] == 1, "every pair NaN: no edge, one empty pass, and the call ends"


# ---- 5. the matrix kernel's bits ---------------------------------------------------------------------------------------------------------
def test_edge_distances_are_the_matrix_kernels_bits():
    from hulk_amd.smash import distance_matrix
    for kind, arg, metric in (("random_set", 33, "weightedjaccard"), ("random_set", 33, "jaccard"), ("weighted_set", None, "weightedjaccard"),
                              ("planted_chains", 512, "weightedjaccard")):
        mins, weights, D = di.named_set(kind, arg, metric)
        M = distance_matrix(mins, weights, metric)
        (a, b, d), _ = run(mins, weights, metric, 96)
        assert len(a) and np.array_equal(di.bits(d), di.bits(np.fmin(M[a, b], M[b, a]))), (kind, arg, metric)


# ---- 6. a cut is a clustering ----------------------------------------------------------------------------------------------------------
def test_cut_equals_cluster():
    from hulk_amd.smash import cluster, cut_dendrogram
    cases = []
    for metric in di.METRICS:
        cases += [("random_set", 33, metric, t) for t in ci.random_set(33)[2][metric][1]]
    for s in (8, 33):
        tau = ci.chain_tau(s)
        cases += [("planted_chains", s, "jaccard", tau), ("planted_chains", s, "jaccard", float(np.nextafter(tau, 0.0)))]
    trees = {}
    for kind, arg, metric, tau in cases:
        mins, weights, D = di.named_set(kind, arg, metric)
        if (kind, arg, metric) not in trees:
            trees[(kind, arg, metric)] = run(mins, weights, metric)[0]
        a, b, d = trees[(kind, arg, metric)]
        labels, n_clusters = cut_dendrogram(len(mins), a, b, d, tau)
        want = cluster(mins, weights, tau, metric)
        assert np.array_equal(labels, want[0]) and n_clusters == want[1], (kind, arg, metric, tau)
        assert np.array_equal(labels, ci.components(D, tau)[0])


# ---- 7. invariance -----------------------------------------------------------------------------------------------------------------------
def test_bands_and_repeats_do_not_change_a_byte_and_a_search_is_what_it_was():
    from hulk_amd.smash import search
    mins, weights, per_metric = ci.random_set(33)
    for metric in di.METRICS:
        before = search(mins[:65], weights[:65], mins, weights, 5, metric, "row")
        first = None
        for band, bands in zip(ci.BANDS, (1, 9, 3)):
            for _ in range(2):
                (a, b, d), st = run(mins, weights, metric, band)
                assert st["bands"] == bands
                got = (a.tobytes(), b.tobytes(), d.tobytes(), st["rounds"], st["edges"], st["components"])
                first = first or got
                assert got == first, f"{metric} band_rows {band}"
        after = search(mins[:65], weights[:65], mins, weights, 5, metric, "row")
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---- 8. the directory form and the CLI -------------------------------------------------------------------------------------------------
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


def render_csv(order, a, b, d):
    from hulk_amd.smash import go_csv_field, go_format_f2
    parent, size = list(range(len(order))), [1] * len(order)

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    out = "merge,sketch_a,sketch_b,distance,similarity,size\n"
    for k, (x, y, h) in enumerate(zip(a.tolist(), b.tolist(), d.tolist())):
        rx, ry = find(x), find(y)
        parent[max(rx, ry)] = min(rx, ry)
        size[min(rx, ry)] = size[rx] + size[ry]
        out += f"{k + 1},{go_csv_field(order[x])},{go_csv_field(order[y])},{h:.17g},{go_format_f2(100 - (h * 100))},{size[min(rx, ry)]}\n"
    return out


def test_directory_form_and_cli(tmp_path):
    """40 sketch files out of the planted chains (one with a comma in its name): dendrogram_files gives the array form's edges in
    sorted path order and writes the CSV a Python rendering gives, every distance reads back to the same double; with a cut the
    clusters file is cluster_files' at that max_distance, byte for byte; the CLI writes the same files and logs the counts"""
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
        want, want_st = run(mins[at], weights[at], metric)
        assert_same(want, di.kruskal(pyorc.smash_matrix(mins[at], weights[at], metric)), metric)
        out, cut_out, ref_out = (str(tmp_path / f"{x}_{metric}.csv") for x in ("py", "cut", "cluster"))
        st = {}
        got_order, a, b, h = smash.dendrogram_files([str(d / n) for n in names] + [str(d / names[0])], metric=metric, csv_path=out,
                                                    cut_distance=t, cut_csv_path=cut_out, stats=st)
        assert got_order == order
        assert_same((a, b, h), want, f"files {metric}")
        assert st["edges"] == len(a) == 39 and st["components"] == 1 and st["bands"] == 1 and st["rounds"] == want_st["rounds"]
        text = open(out).read()
        assert text == render_csv(order, a, b, h), text
        assert '"' + str(d / "s,03.json") + '"' in text
        rows = [line.rsplit(",", 3) for line in text.splitlines()[1:]]
        assert [float(r[1]) for r in rows] == h.tolist() and int(rows[-1][3]) == 40, "%.17g reads back to the same double"
        smash.cluster_files([str(d / n) for n in names], t, metric=metric, csv_path=ref_out)
        assert open(cut_out, "rb").read() == open(ref_out, "rb").read()
        if metric == "jaccard":
            assert 1 < smash.cut_dendrogram(40, a, b, h, t)[1] < 40, ci.NO_TEST + "the cut"
        r = cli(["dendrogram", "-d", str(d), "-m", metric, "--cut", repr(t), "-o", str(tmp_path / "cli")])
        assert r.returncode == 0 and "HULK DENDROGRAM!" in r.stdout, r.stdout + r.stderr
        assert open(str(tmp_path / "cli") + ".hulk-dendrogram.csv").read() == text
        assert open(str(tmp_path / "cli") + ".hulk-clusters.csv", "rb").read() == open(ref_out, "rb").read()
        c = cli(["cluster", "-d", str(d), "-m", metric, "--maxDistance", repr(t), "-o", str(tmp_path / "ref")])
        assert c.returncode == 0 and open(str(tmp_path / "ref") + ".hulk-clusters.csv", "rb").read() == open(ref_out, "rb").read()
        for line in ("number of sketches: 40", "number of edges: 39", "number of components: 1", f"number of rounds: {st['rounds']}",
                     f"largest merge height: {float(h[-1])!r}"):
            assert line in r.stdout, (line, r.stdout)
    # --cutSimilarity 75 is --cut 0.25; without a cut no clusters file is written
    assert tau == 0.25
    x = cli(["dendrogram", "-d", str(d), "--cutSimilarity", "75", "-o", str(tmp_path / "sim")])
    y = cli(["dendrogram", "-d", str(d), "-o", str(tmp_path / "plain")])
    assert x.returncode == 0 and y.returncode == 0, x.stdout + y.stdout
    assert open(str(tmp_path / "sim") + ".hulk-clusters.csv").read() == open(str(tmp_path / "cluster_jaccard.csv")).read()
    assert open(str(tmp_path / "plain") + ".hulk-dendrogram.csv").read() == open(str(tmp_path / "py_jaccard.csv")).read()
    assert not os.path.exists(str(tmp_path / "plain") + ".hulk-clusters.csv")
    # one file is a set; MinHash signatures carry no weights: jaccard works, weightedjaccard is the reference's refusal
    one_order, a, b, h = smash.dendrogram_files([str(d / names[0])])
    assert one_order == [str(d / names[0])] and len(a) == len(b) == len(h) == 0
    for algo in ("khf", "kmv"):
        m = tmp_path / algo
        m.mkdir()
        for i in range(12):
            write_sketch(str(m / f"m{i:02d}.json"), mins[i], None, algo=algo)
        out = str(tmp_path / f"{algo}.csv")
        got_order, a, b, h = smash.dendrogram_files([str(p) for p in m.iterdir()], algo=algo, csv_path=out)
        assert_same((a, b, h), di.kruskal(pyorc.smash_matrix(mins[:12], np.zeros((12, s)), "jaccard")), algo)
        assert open(out).read() == render_csv(got_order, a, b, h)
        r = cli(["dendrogram", "-d", str(m), "-a", algo, "-m", "weightedjaccard", "-o", str(tmp_path / algo / "w")])
        assert r.returncode == 1 and "weighted jaccard is only supported for histosketches" in r.stdout


# ---- 9. the C++ host ---------------------------------------------------------------------------------------------------------------------
def test_cpp_host_matches_the_python_binding(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    exe = str(tmp_path / "dendrogram_driver")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "dendrogram_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    s = 33
    mins, weights, per_metric = ci.random_set(s)
    path = str(tmp_path / "sketches.txt")
    with open(path, "w") as fh:
        for a, b in zip(mins, weights):
            fh.write(" ".join([str(int(v)) for v in a] + [float(v).hex() for v in b]) + "\n")
    for metric, band in (("jaccard", 0), ("weightedjaccard", 96), ("jaccard", 32)):
        r = subprocess.run([exe, path, str(s), metric, str(band)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        (a, b, d), st = run(mins, weights, metric, band)
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(a) + 1
        got = [line.split() for line in lines[:-1]]
        assert all(g[0] == "edge" for g in got)
        assert [int(g[1]) for g in got] == a.tolist() and [int(g[2]) for g in got] == b.tolist()
        assert [float.fromhex(g[3]) for g in got] == d.tolist()
        assert lines[-1] == f"stats {st['rounds']} {st['bands']} {st['edges']} {st['components']}"
    r = subprocess.run([exe, path, str(s), "jaccard", "33"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("hulk::Error -30|") and "band_rows must be a multiple of 32" in r.stdout
