"""The bottom-k metric (HULK_METRIC_BOTTOMK) on the GPU, bit for bit (== on the doubles) against the yardstick of
tests/bottomk_inputs.py, which is KMVsketch.GetSimilarity (kmv.go:119-159) restated.

Planted pairs with the intersection worked out by hand, alone (N = 2) and inside sets of 33, 65 and 97 sketches, at S = 1, 2, 31, 33,
50 and 512; the largest sketch the metric takes (4096) and the smallest; the order of a sketch's values; N around the tile's 32 and
64; and the four users of the tile — hulk_smash's matrix, hulk_search, hulk_cluster, hulk_dendrogram — on one collection full of ties;
and `sketch --kmv --feedMinHash` to `smash -a kmv -m bottomk` end to end.  Shapes are the smallest that can break the kernels.

Above one position per thread of the preparation the sizes are ragged on purpose — 257, 513, 1000, 2049, 4095 (bottomk_inputs.RAGGED_SIZES):
the planted pairs and sets at each, the four orders of a sketch's values at 1000, every user of the tile (links and the three
linkages too) at 2049 with the closest pair's distance followed through all of them, and a set of lists of 1 .. S distinct values."""
import functools
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import bottomk_inputs as bi
import cluster_inputs as ci
import dendrogram_inputs as di
import linkage_inputs as lni
import links_inputs as lki
from conftest import pack_reads
from test_gpu_cluster import assert_same as assert_same_clusters, run as run_cluster
from test_gpu_dendrogram import assert_same as assert_same_edges, run as run_dendrogram
from test_gpu_linkage import assert_same as assert_same_merges, run as run_linkage
from test_gpu_links import run as run_links
from test_gpu_search import assert_hits, bits, select

pytestmark = pytest.mark.gpu


def gpu_matrix(mins, metric="bottomk", weights=None):
    from hulk_amd.smash import distance_matrix
    return distance_matrix(mins, weights, metric)


def assert_matrix(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} distances differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


@functools.lru_cache(maxsize=None)
def planted_reference(n, s):
    m = bi.planted_set(n, s)
    D = bi.matrix(m, sample=300 if s <= 512 else 100)               # (the pairs the yardstick's two forms are compared on)
    m.setflags(write=False); D.setflags(write=False)
    return m, D


@pytest.mark.parametrize("s", [1, 2, 31, 33, 50, 512])
def test_planted_pairs(s):
    planted(s, (33, 65, 97))


@pytest.mark.parametrize("s", bi.RAGGED_SIZES)
def test_planted_pairs_at_ragged_sizes(s):
    """S = 257 .. 4095: k_bottomk_prep finds the run heads with E = 2 .. 16 positions a thread, the last threads own a partial range or
    none, and the network skips every comparator whose upper end is not below S (tests/bottomk_inputs.py: check_ragged_sizes)"""
    planted(s, (33, 65))


def planted(s, ns):
    from oracle import pyorc
    for name, a, b, want in bi.planted_pairs(s):
        m = np.vstack([a, b])
        D = gpu_matrix(m)
        d = 1.0 - float(want) / float(s)
        print(f"S {s} {name}: intersect {want}, distance {D[0, 1]!r}")
        assert D[0, 1] == d == D[1, 0] == bi.distance(a, b), (s, name, D.tolist(), d)
        assert D[0, 0] == 0.0 == D[1, 1], (s, name, D.tolist())
        if name == "shifted by one rank":
            # the two sorted lists position by position, what `-m jaccard` compares: nothing in common.  The metrics differ
            srt = np.vstack([np.sort(a), np.sort(b)])
            J = gpu_matrix(srt, "jaccard", np.zeros(srt.shape))
            assert J[0, 1] == 1.0 == pyorc.smash_matrix(srt, np.zeros(srt.shape), "jaccard")[0, 1] and D[0, 1] == 1.0 - (s - 1) / s
            assert_matrix(gpu_matrix(srt), D, f"S {s} {name}, sorted")
    for n in ns:
        m, want = planted_reference(n, s)
        assert_matrix(gpu_matrix(m), want, f"N {n} S {s} planted set")


def test_the_largest_and_the_smallest_sketch():
    s = 4096
    pairs = bi.planted_pairs(s)
    rows = [pairs[0][1], pairs[0][2], pairs[2][2], pairs[-2][1], pairs[-2][2]]      # identical, shifted, runs across the preparation's boundaries
    m = np.array(rows, dtype=np.uint64)
    assert m.shape == (5, s)
    assert_matrix(gpu_matrix(m), bi.matrix(m, sample=25), "N 5 S 4096")
    m = bi.random_set(5, s, 4096, spread=1)                         # long runs: about a third of the values are distinct
    assert_matrix(gpu_matrix(m), bi.matrix(m, sample=25), "N 5 S 4096, runs")
    m = np.array([[5], [5], [6], [bi.U64_MAX], [0], [bi.U64_MAX]], dtype=np.uint64)
    D = gpu_matrix(m)
    assert_matrix(D, bi.matrix(m), "N 6 S 1")
    assert D[0, 1] == 0.0 and D[0, 2] == 1.0 and D[3, 5] == 0.0 and D[3, 4] == 1.0


@pytest.mark.parametrize("s", [50, 512, 1000])
def test_the_order_of_a_sketchs_values_does_not_matter(s):
    m = bi.random_set(70, s, 31 + s)
    want = bi.matrix(m)
    rng = np.random.default_rng(s)
    forms = {"as drawn": m, "permuted": np.array([rng.permutation(r) for r in m]), "ascending": np.sort(m, axis=1),
             "descending": np.sort(m, axis=1)[:, ::-1].copy()}
    for name, f in forms.items():
        assert_matrix(gpu_matrix(f), want, f"N 70 S {s} {name}")


def test_tile_borders():
    """N one below, at and one above the multiples of the tile's 32 subjects and 64 others: every pair inside the set is right, and no
    pair outside it is counted — the links of a clustering at tau = 1 are all N * (N - 1) ordered pairs, a self search finds N - 1 hits"""
    from hulk_amd.smash import search
    c = bi.tile_constants()
    s = 50
    full = bi.random_set(2 * c["TQ"] + 1, s, 50)
    want_full = bi.matrix(full)
    ns = sorted({x for k in (1, 2, 3, 4) for x in (k * c["TS"] - 1, k * c["TS"], k * c["TS"] + 1)} | {1, 2})
    assert ns[-1] == len(full)
    for n in ns:
        m, want = full[:n], want_full[:n, :n]
        assert_matrix(gpu_matrix(m), want, f"N {n} S {s}")
        labels, links, clusters = run_cluster(m, None, 1.0, "bottomk")
        assert links == n * (n - 1) and clusters == 1 and (labels == 0).all(), (n, links, clusters)
        if n > 1:
            got = search(m, None, None, None, 64, "bottomk", self_search=True)
            assert_hits(got, select(want, 64, no_diagonal=True), f"N {n} S {s} self search")
            assert (got[2] == min(n - 1, 64)).all()


def collection(s):
    """130 sketches whose values come from a small range: ties between pairs abound (tests/bottomk_inputs.py checks that they do)"""
    return bi.tied_collection(s)


def bi_no_test(why):
    return bi.NO_TEST + why


@pytest.mark.parametrize("s", [50, 512])
def test_the_four_users_agree(s):
    four_users(s)


def test_every_user_of_the_tile_agrees_at_2049():
    """S = 2049 (nine positions a thread of the preparation, a ragged end) through the matrix, search, cluster, dendrogram — as at 50 and
    512 — and links and the three linkages; the closest pair of the collection is one distance, and it has the same bits wherever a
    user reports it"""
    from hulk_amd.smash import search
    s = 2049
    four_users(s)
    m, D = collection(s)
    n = len(m)
    a, b = bi.closest_pair(D)
    seen = {"yardstick": bits(D[a, b]).item(), "matrix": bits(gpu_matrix(m)[a, b]).item()}
    index, dist, count = search(m, None, None, None, 1, "bottomk", self_search=True)
    assert index[a, 0] == b and count[a] == 1
    seen["search"] = bits(dist[a, 0]).item()
    tau = float(D[a, b])
    for band in (32, 0):
        got = run_links(m, None, tau, "bottomk", band)
        lki.assert_same(got, lki.csr(D, tau), f"N {n} S {s} links at tau {tau!r} band_rows {band}")
    ptr, idx, ld = got
    row = idx[int(ptr[a]):int(ptr[a + 1])].tolist()
    assert row[0] == b and int(ptr[-1]) >= 2, "at the smallest distance of the set a's first link is b"
    seen["links"] = bits(ld[int(ptr[a])]).item()
    off = np.unique(D[~np.eye(n, dtype=bool)])
    mid = float(off[len(off) // 8])
    lki.assert_same(run_links(m, None, mid, "bottomk", 32), lki.csr(D, mid), f"N {n} S {s} links at tau {mid!r}")
    (ea, eb, ed), _ = run_dendrogram(m, None, "bottomk", 0)
    assert (int(ea[0]), int(eb[0])) == (a, b)
    seen["dendrogram"] = bits(ed[0]).item()
    for method in lni.METHODS:
        got, _ = run_linkage(m, None, method, "bottomk")
        assert_same_merges(got, lni.agglomerate(D, method), f"N {n} S {s} {method} linkage")
        assert (int(got[0][0]), int(got[1][0])) == (a, b)
        seen[method] = bits(got[2][0]).item()
    print(f"S {s}: the closest pair ({a}, {b}) at {D[a, b]!r} as {sorted(seen)}")
    assert len(set(seen.values())) == 1 and len(seen) == 8, seen


def test_lists_of_very_different_density():
    """a list of S copies of one value, a list of S distinct values, MaxUint64 and 0 S times over, and a ladder of densities between
    them at S = 1000: the tile's windows advance at very different rates (many short rounds) and stay exact"""
    from hulk_amd.smash import search
    n, s = 40, 1000
    m, D = bi.check_density_set(n, s)
    assert_matrix(gpu_matrix(m), D, f"N {n} S {s} density set")
    assert_matrix(gpu_matrix(np.sort(m, axis=1)), D, f"N {n} S {s} density set, ascending")
    assert_hits(search(m, None, None, None, 33, "bottomk", self_search=True), select(D, 33, no_diagonal=True), f"N {n} S {s} density set, self search")
    for tau in (0.5, 1.0 - 1.0 / s):
        assert_same_clusters(run_cluster(m, None, tau, "bottomk"), ci.components(D, tau), f"N {n} S {s} density set, tau {tau!r}")


def four_users(s):
    from hulk_amd.smash import search
    m, D = collection(s)
    n = len(m)
    assert_matrix(gpu_matrix(m), D, f"N {n} S {s} matrix")
    # search: among themselves, and against a database that comes in several strips; role is ignored
    for role in ("row", "column"):
        got = search(m, None, None, None, 64, "bottomk", role, self_search=True)
        assert_hits(got, select(D, 64, no_diagonal=True), f"N {n} S {s} self search ({role})")
    q = m[:40]
    for k, lim in ((5, None), (64, float(np.median(D)))):
        st = {}
        got = search(q, None, m, None, k, "bottomk", max_distance=lim, scratch_bytes=64 * (s * 32 + 64 * 8), stats=st)
        assert st["strips"] == 3, st
        assert_hits(got, select(D[:40], k, max_distance=lim), f"N {n} S {s} K {k} search in {st['strips']} strips")
    # cluster: thresholds that are distances of the set (equality links), and one between two of them
    off = np.unique(D[~np.eye(n, dtype=bool)])
    taus = [float(off[len(off) // 8]), float(off[len(off) // 4]), float((off[len(off) // 6] + off[len(off) // 6 + 1]) / 2)]
    wants = {}
    for tau in taus:
        wants[tau] = ci.components(D, tau)
        print(f"S {s}: tau {tau!r}, {wants[tau][1]} links, {wants[tau][2]} clusters")
        for band in (32, 0):
            assert_same_clusters(run_cluster(m, None, tau, "bottomk", band), wants[tau], f"N {n} S {s} tau {tau!r} band_rows {band}")
    assert len({w[2] for w in wants.values()}) == 3 and all(w[1] > 0 and w[2] > 1 for w in wants.values()), bi_no_test("the thresholds cut nothing")
    # dendrogram: Kruskal on the yardstick's matrix, in several bands and in one; every cut is the clustering
    want_edges = di.kruskal(D)
    for band in (32, 0):
        (a, b, d), st = run_dendrogram(m, None, "bottomk", band)
        assert_same_edges((a, b, d), want_edges, f"N {n} S {s} dendrogram band_rows {band}")
        assert band == 0 or st["bands"] > 1
        for tau in taus:
            assert np.array_equal(di.cut_labels(n, a, b, d, tau), wants[tau][0]), (s, band, tau)


def _cli(args):
    from hulk_amd.__main__ import main
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main(args)
    return rc, buf.getvalue()


def test_sketch_to_smash_end_to_end(tmp_path, fq_reads):
    """three KMV sketches of the fixture's reads — all of them, the first 800, the last 600 — written as `sketch --kmv --feedMinHash`
    writes them, then `smash -a kmv -m bottomk`: the CSV is the yardstick's strings, the similarities order as the overlaps do; and
    `dendrogram --cut` writes the file `cluster --maxDistance` writes"""
    import hulk_amd
    from hulk_amd import _lib
    from hulk_amd.sketchio import HULKdata
    from hulk_amd.smash import collect_jsons, go_csv_field, go_format_f2
    db = tmp_path / "db"
    db.mkdir()
    subsets = {"a_all": fq_reads, "b_first800": fq_reads[:800], "c_last600": fq_reads[400:]}
    sketches = []
    for name, reads in subsets.items():
        g = hulk_amd.GpuSketcher(21, 9, 256, flags=_lib.HULK_FLAG_KMV)
        g.add_reads(*pack_reads(reads))
        g.finish()
        sk = g.kmv_sketch()
        g.close()
        assert len(sk.mins) == 256
        d = HULKdata(); d.filename, d.banner_label = name + ".fq,", "blank"
        d.add(sk)
        d.write_json(str(db / (name + ".json")))
        sketches.append(sk.mins)
    want = bi.matrix(np.array(sketches, dtype=np.uint64))
    out = str(tmp_path / "out")
    rc, text = _cli(["smash", "-d", str(db), "-o", out, "-a", "kmv", "-m", "bottomk"])
    assert rc == 0, text
    order = sorted(collect_jsons(str(db)))
    lines = [",".join(go_csv_field(f) for f in order)] + [",".join(go_format_f2(100 - (x * 100)) for x in row) for row in want.tolist()]
    got = open(out + ".hulk-matrix.csv").read()
    assert got == "\n".join(lines) + "\n", got
    sim = 100 - want * 100
    print(sim)
    assert (np.diag(sim) == 100).all() and ((sim[~np.eye(3, dtype=bool)] > 0) & (sim[~np.eye(3, dtype=bool)] < 100)).all()
    assert sim[0, 1] > sim[0, 2] > sim[1, 2], "800, 600 and 400 shared reads"
    # position by position the same three lists have next to nothing in common
    rc, text = _cli(["smash", "-d", str(db), "-o", out + "_j", "-a", "kmv", "-m", "jaccard"])
    assert rc == 0 and open(out + "_j.hulk-matrix.csv").read() != got
    tau = repr(float(want[0, 2]))
    rc, text = _cli(["cluster", "-d", str(db), "-o", out + "_c", "-a", "kmv", "-m", "bottomk", "--maxDistance", tau])
    assert rc == 0, text
    rc, text = _cli(["dendrogram", "-d", str(db), "-o", out + "_d", "-a", "kmv", "-m", "bottomk", "--cut", tau])
    assert rc == 0, text
    clusters = open(out + "_c.hulk-clusters.csv").read()
    assert clusters == open(out + "_d.hulk-clusters.csv").read() and clusters.count("\n") == 4
    assert [l.split(",")[1] for l in clusters.splitlines()[1:]] == ["1", "1", "1"], clusters     # a-b and a-c link at d(a, c); b-c need not
