"""Single-, complete- and average-linkage dendrograms of a sketch collection on the GPU (hulk_linkage: the matrix kernel,
k_linkage_sym, k_linkage_pick, k_linkage_update, k_linkage_rescan).

The yardstick throughout is tests/linkage_inputs.py: oracle.pyorc.smash_matrix over the set, W = fmin(D, D.T) (+inf where both
directions are NaN), then the primitive agglomeration with a literal argmin of the key (d, p, q) every step.  Index arrays and sizes
are compared as equal and distances as bits; the "the inputs are no test" conditions of every generator are asserted before anything
is compared."""
import os
import subprocess

import numpy as np
import pytest

import bottomk_inputs as bk
import cluster_inputs as ci
import dendrogram_inputs as di
import linkage_inputs as li
from conftest import ROOT

pytestmark = pytest.mark.gpu


def run(mins, weights, method, metric):
    from hulk_amd.smash import linkage
    st = {}
    a, b, d, size = linkage(mins, weights, method, metric, stats=st)
    n = len(mins)
    assert a.dtype == np.uint32 and b.dtype == np.uint32 and d.dtype == np.float64 and size.dtype == np.uint32
    assert len(a) == len(b) == len(d) == len(size) == st["merges"] and st["components"] == n - len(a), st
    assert (a < b).all() and (b < n).all()
    assert st["rows_rescanned"] >= (n if n > 1 else 0) + len(a), "the first fill scans every row, every merge at least row p"
    return (a, b, d, size), st


def assert_same(got, want, what):
    ga, gb, gd, gs = got
    wa, wb, wd, ws = want
    assert len(ga) == len(wa), f"{what}: {len(ga)} merges, want {len(wa)}"
    bad = np.nonzero((ga != wa) | (gb != wb) | (li.bits(gd) != li.bits(wd)) | (gs != ws))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} merges differ, first at {bad[:3].tolist()}: got "
                           f"{[(int(ga[i]), int(gb[i]), float(gd[i]).hex(), int(gs[i])) for i in bad[:3]]}, want "
                           f"{[(int(wa[i]), int(wb[i]), float(wd[i]).hex(), int(ws[i])) for i in bad[:3]]}")


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 8, 33])
def test_shapes(s):
    """N: one sketch, two, a tile of 32 less one, exactly, plus one, 64 less one, exactly, plus one, 257 (a tail behind eight tiles of
    k_linkage_sym, two workgroups of k_linkage_update, seventeen groups of k_linkage_rescan); S = 1 under jaccard has the distances
    0 and 1 alone: every step is decided by the key's tie rule.  Every smaller set is the first N sketches of the 257."""
    kind, arg = di.shapes_set(s)
    for metric in li.METRICS:
        mins, weights, D = li.named_set(kind, arg, metric)
        for n in ci.NS:
            for method in li.METHODS:
                got, st = run(mins[:n], weights[:n], method, metric)
                assert_same(got, li.reference(kind, arg, metric, method, n), f"N {n} S {s} {metric} {method}")
                if n == 1:
                    assert st["merges"] == 0 and st["components"] == 1
        print(f"S {s} {metric}: heights at N = 257 {[(m, li.reference(kind, arg, metric, m)[2][[0, -1]].tolist()) for m in li.METHODS]}")


# ---- 2. the strided loops -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", li.METRICS)
def test_grid_stride_paths(metric):
    """N = 1,100: above the 1,024 lanes of k_linkage_pick's workgroup and four times k_linkage_rescan's 256 — every strided loop
    runs more than once"""
    mins, weights, D = li.named_set("grid_set", None, metric)
    for method in li.METHODS:
        got, st = run(mins, weights, method, metric)
        assert_same(got, li.reference("grid_set", None, metric, method), f"N {li.GRID_N} {metric} {method}")
        print(f"{metric} {method}: {st['merges']} merges, {st['rows_rescanned'] / max(st['merges'], 1):.2f} rows rescanned per merge, "
              f"matrix {st['kernel_ms_matrix']:.3f} ms, merges {st['kernel_ms_merge']:.3f} ms")


# ---- 3. directions, NaN, Inf ---------------------------------------------------------------------------------------------------------
def test_weighted_directions_nan_and_a_forest():
    clusters_left = li.check_weighted_forest()
    mins, weights, D = li.weighted_forest_set()
    W = li.weights_matrix(D)
    for method in li.METHODS:
        got, st = run(mins, weights, method, "weightedjaccard")
        assert_same(got, li.agglomerate(D, method), f"the weighted forest set, {method}")
        assert st["components"] == clusters_left[method] == len(mins) - st["merges"]
        assert not [m for m in li.member_sets(len(mins), got[0], got[1]) if ci.Z in m and li.Z2 in m] or method == "single"
    assert clusters_left["single"] == li.finite_components(D) and clusters_left["complete"] > 1
    # the merge of the two singletons X0, X1 (nothing else is near either) is at the smaller direction's bits
    (a, b, d, size), _ = run(mins, weights, "complete", "weightedjaccard")
    at = {(int(x), int(y)): h for x, y, h in zip(a, b, d)}
    assert li.bits(at[(ci.X0, ci.X1)]) == li.bits(D[ci.X0, ci.X1]) != li.bits(D[ci.X1, ci.X0]), "the smaller direction's bits"
    assert at[(ci.I0, ci.I1)] == 0 and W[ci.U, ci.V] == D[ci.V, ci.U]
    # cluster_inputs' own weighted set (no pair is NaN both ways), under both metrics
    for metric in li.METRICS:
        mins, weights, D = li.named_set("weighted_set", None, metric)
        for method in li.METHODS:
            got, st = run(mins, weights, method, metric)
            assert_same(got, li.reference("weighted_set", None, metric, method), f"weighted_set {metric} {method}")


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------------------
def test_ties_stars_and_a_set_without_any_merge():
    li.check_stars()
    for kind, h in (("identical_set", 0.0), ("disjoint_set", 1.0)):
        for metric in li.METRICS:
            mins, weights, D = li.named_set(kind, None, metric)
            for method in li.METHODS:
                (a, b, d, size), st = run(mins, weights, method, metric)
                assert not a.any() and b.tolist() == list(range(1, 65)) and size.tolist() == list(range(2, 66)), (kind, metric, method)
                assert (li.bits(d) == li.bits(np.full(64, h))).all() and st["components"] == 1
    mins, weights = di.zero_weight_set()
    for method in li.METHODS:
        (a, b, d, size), st = run(mins, weights, method, "weightedjaccard")
        assert len(a) == 0 and st["merges"] == 0 and st["components"] == 3, "every pair NaN: no merge, and the call ends"


# ---- 5. single linkage is the dendrogram and the clustering ---------------------------------------------------------------------------------
def test_single_linkage_is_the_spanning_forest_and_every_cut_a_clustering():
    from hulk_amd.smash import cluster, cut_dendrogram, dendrogram
    for kind, arg, metric in (("random_set", 33, "weightedjaccard"), ("random_set", 8, "jaccard"), ("planted_chains", 8, "jaccard")):
        mins, weights, D = li.named_set(kind, arg, metric)
        (a, b, d, size), _ = run(mins, weights, "single", metric)
        ea, eb, ed = dendrogram(mins, weights, metric)
        assert np.array_equal(np.sort(li.bits(d)), np.sort(li.bits(ed))), "the heights are hulk_dendrogram's edge distances as a multiset of bits"
        assert (np.diff(d) >= 0).all()
        taus = [0.0, 1.0, ci.chain_tau(8), float(np.nextafter(ci.chain_tau(8), 0.0))]
        taus += ci.random_set(arg)[2][metric][1] if kind == "random_set" else []
        for tau in taus:
            labels, k = cut_dendrogram(len(mins), a, b, d, tau)
            want = cluster(mins, weights, tau, metric)
            assert np.array_equal(labels, want[0]) and k == want[1], (kind, arg, metric, tau)


# ---- 6. complete linkage ------------------------------------------------------------------------------------------------------------------
def test_complete_linkage_heights_are_the_largest_distance_inside_the_cluster():
    from hulk_amd.smash import distance_matrix
    tau = li.check_complete_differs_from_single()
    for kind, arg, metric in (("random_set", 33, "weightedjaccard"), ("planted_chains", 8, "jaccard")):
        mins, weights, D = li.named_set(kind, arg, metric)
        M = distance_matrix(mins, weights, metric)
        W = np.fmin(M, M.T)
        W[np.isnan(W)] = np.inf
        (a, b, d, size), _ = run(mins, weights, "complete", metric)
        assert (np.diff(d) >= 0).all(), "heights never step down"
        for members, h, sz in zip(li.member_sets(len(mins), a, b), d, size):
            m = np.array(sorted(members))
            sub = W[np.ix_(m, m)][np.triu_indices(len(m), 1)]
            assert len(m) == sz and li.bits(h) == li.bits(sub.max()), (kind, arg, metric)
    # ... and at the chains' threshold it does not chain
    mins, weights, D = li.named_set("planted_chains", 8, "jaccard")
    (a, b, d, size), _ = run(mins, weights, "complete", "jaccard")
    (sa, sb, sd, ss), _ = run(mins, weights, "single", "jaccard")
    assert not np.array_equal(di.cut_labels(257, a, b, d, tau), di.cut_labels(257, sa, sb, sd, tau))


# ---- 7. repeatability -----------------------------------------------------------------------------------------------------------------------
def test_repeats_do_not_change_a_byte_and_smash_is_what_it_was():
    from hulk_amd.smash import distance_matrix
    mins, weights, per_metric = ci.random_set(33)
    for metric in li.METRICS:
        before = distance_matrix(mins, weights, metric)
        for method in li.METHODS:
            first = None
            for _ in range(2):
                (a, b, d, size), st = run(mins, weights, method, metric)
                got = (a.tobytes(), b.tobytes(), d.tobytes(), size.tobytes(), st["merges"], st["components"], st["rows_rescanned"])
                first = first or got
                assert got == first, f"{metric} {method}"
        after = distance_matrix(mins, weights, metric)
        assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
        assert np.array_equal(before.view(np.uint64), np.asarray(per_metric[metric][0]).view(np.uint64))


# ---- 8. bottomk -------------------------------------------------------------------------------------------------------------------------------
def test_bottomk():
    mins = bk.random_set(70, 16, 4100)
    D = bk.matrix(mins)
    for method in li.METHODS:
        got, st = run(mins, None, method, "bottomk")
        want = li.agglomerate(D, method)
        assert len(want[0]) and len(np.unique(want[2])) < len(want[2]), li.NO_TEST + "no merges or no ties"
        assert_same(got, want, f"bottomk {method}")


# ---- 9. the directory form and the CLI --------------------------------------------------------------------------------------------------
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


def render_csv(order, a, b, d, size):
    from hulk_amd.smash import go_csv_field, go_format_f2
    out = "merge,sketch_a,sketch_b,distance,similarity,size\n"
    for k, (x, y, h, s) in enumerate(zip(a.tolist(), b.tolist(), d.tolist(), size.tolist())):
        out += f"{k + 1},{go_csv_field(order[x])},{go_csv_field(order[y])},{h:.17g},{go_format_f2(100 - (h * 100))},{s}\n"
    return out


def render_clusters(order, labels):
    from hulk_amd.smash import go_csv_field
    ordinal, nxt = {}, 0
    for i, l in enumerate(labels.tolist()):
        if l == i:
            nxt += 1
            ordinal[i] = nxt
    sizes = np.bincount(labels, minlength=len(order))
    out = "sketch,cluster,size,representative\n"
    for i, l in enumerate(labels.tolist()):
        out += f"{go_csv_field(order[i])},{ordinal[l]},{sizes[l]},{go_csv_field(order[l])}\n"
    return out


def test_directory_form_and_cli(tmp_path):
    """40 sketch files out of the planted chains (one with a comma in its name): linkage_files gives the yardstick's merges in sorted
    path order and writes the CSV a Python rendering of the yardstick gives; with a cut the clusters file is cut_dendrogram's; the
    CLI writes the same files with --linkage, and without it takes the single-linkage path it always took"""
    from hulk_amd import smash
    from oracle import pyorc
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
    for metric, method, t in (("jaccard", "complete", 2 * tau), ("weightedjaccard", "average", 0.9), ("jaccard", "single", tau)):
        want = li.agglomerate(pyorc.smash_matrix(mins[at], weights[at], metric), method)
        out, cut_out = (str(tmp_path / f"{x}_{metric}_{method}.csv") for x in ("py", "cut"))
        st = {}
        got_order, a, b, h, size = smash.linkage_files([str(d / n) for n in names] + [str(d / names[0])], method, metric=metric, csv_path=out,
                                                       cut_distance=t, cut_csv_path=cut_out, stats=st)
        assert got_order == order
        assert_same((a, b, h, size), want, f"files {metric} {method}")
        assert st["merges"] == len(a) == 39 and st["components"] == 1
        text = open(out).read()
        assert text == render_csv(order, *want), text
        assert '"' + str(d / "s,03.json") + '"' in text
        labels, k = smash.cut_dendrogram(40, want[0], want[1], want[2], t)
        assert open(cut_out).read() == render_clusters(order, labels)
        assert 1 < k < 40, ci.NO_TEST + "the cut"
        if method == "single":
            continue
        r = cli(["dendrogram", "-d", str(d), "-m", metric, "--linkage", method, "--cut", repr(t), "-o", str(tmp_path / "cli")])
        assert r.returncode == 0 and "HULK DENDROGRAM!" in r.stdout, r.stdout + r.stderr
        assert open(str(tmp_path / "cli") + ".hulk-dendrogram.csv").read() == text
        assert open(str(tmp_path / "cli") + ".hulk-clusters.csv").read() == render_clusters(order, labels)
        for line in ("number of sketches: 40", "number of merges: 39", "number of components: 1", f"linkage: {method}",
                     f"number of clusters at the cut: {k}", f"largest merge height: {float(h.max())!r}"):
            assert line in r.stdout, (line, r.stdout)
    # --linkage single is the default: the minimum spanning forest's file, not the agglomeration's
    x = cli(["dendrogram", "-d", str(d), "--linkage", "single", "-o", str(tmp_path / "single")])
    y = cli(["dendrogram", "-d", str(d), "-o", str(tmp_path / "plain")])
    assert x.returncode == 0 and y.returncode == 0 and "number of rounds" in x.stdout, x.stdout + y.stdout
    assert open(str(tmp_path / "single") + ".hulk-dendrogram.csv").read() == open(str(tmp_path / "plain") + ".hulk-dendrogram.csv").read()
    ea, eb, ed = smash.dendrogram_files([str(d / n) for n in names])[1:]
    assert open(str(tmp_path / "plain") + ".hulk-dendrogram.csv").read().count("\n") == len(ea) + 1
    # one file is a set; bottomk is for kmv sketches alone
    one = smash.linkage_files([str(d / names[0])], "complete")
    assert one[0] == [str(d / names[0])] and all(len(x) == 0 for x in one[1:])
    for algo in ("khf", "kmv"):
        m = tmp_path / algo
        m.mkdir()
        for i in range(12):
            write_sketch(str(m / f"m{i:02d}.json"), mins[i], None, algo=algo)
        r = cli(["dendrogram", "-d", str(m), "-a", algo, "-m", "bottomk", "--linkage", "complete", "-o", str(m / "w")])
        if algo == "khf":
            assert r.returncode == 1 and "bottomk is only supported for kmv sketches" in r.stdout, r.stdout
        else:
            assert r.returncode == 0, r.stdout + r.stderr
            got = smash.linkage_files([str(p) for p in m.iterdir() if p.suffix == ".json"], "complete", algo="kmv", metric="bottomk")
            assert_same(got[1:], li.agglomerate(bk.matrix(mins[:12]), "complete"), "kmv files under bottomk")


# ---- 10. the C++ host --------------------------------------------------------------------------------------------------------------------
def test_cpp_host_matches_the_python_binding(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    exe = str(tmp_path / "linkage_driver")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "linkage_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    s = 33
    mins, weights, per_metric = ci.random_set(s)
    path = str(tmp_path / "sketches.txt")
    with open(path, "w") as fh:
        for a, b in zip(mins, weights):
            fh.write(" ".join([str(int(v)) for v in a] + [float(v).hex() for v in b]) + "\n")
    for metric, method in (("jaccard", "complete"), ("weightedjaccard", "average"), ("jaccard", "single")):
        r = subprocess.run([exe, path, str(s), metric, method], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        (a, b, d, size), st = run(mins, weights, method, metric)
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(a) + 1
        got = [line.split() for line in lines[:-1]]
        assert all(g[0] == "merge" for g in got)
        assert [int(g[1]) for g in got] == a.tolist() and [int(g[2]) for g in got] == b.tolist() and [int(g[4]) for g in got] == size.tolist()
        assert [float.fromhex(g[3]) for g in got] == d.tolist()
        assert lines[-1] == f"stats {st['merges']} {st['components']} {st['rows_rescanned']}"
    r = subprocess.run([exe, path, str(s), "jaccard", "ward"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("hulk::Error -30|") and "supplied linkage is not available: ward" in r.stdout
