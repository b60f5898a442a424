"""Nearest-neighbour search of sketches against a database on the GPU (hulk_search: k_search_dist, k_search_select).

The yardstick throughout is oracle.pyorc.smash_matrix over the stack [queries; database], as in tests/test_gpu_panel.py: block
[:m, m:] for role "row", [m:, :m].T for role "column"; then the selection in numpy — mask NaN and the values above max_distance,
np.lexsort((index, distance)), the first K (tests/search_inputs.py).  Indices are compared exactly, distances on the uint64 view,
and behind count[i] the entries must be 0xFFFFFFFF / NaN."""
import functools
import os
import subprocess

import numpy as np
import pytest

import search_inputs as si
from conftest import ROOT
from search_inputs import NONE, bits, blocks, select          # (the yardstick: one definition, the tests of other modules import it from here)
from test_gpu_panel import make_sketches

pytestmark = pytest.mark.gpu

VARIANTS = [("jaccard", "row"), ("jaccard", "column"), ("weightedjaccard", "row"), ("weightedjaccard", "column")]
MS, PS, KS = (1, 31, 32, 33, 65), (1, 63, 64, 65, 257), (1, 5, 64)
MAXF = 1.7976931348623157e308


def assert_hits(got, want, what):
    gi, gd, gc = got
    wi, wd, wc = want
    assert gi.shape == wi.shape and gd.shape == wd.shape, what
    assert np.array_equal(gc, wc), f"{what}: counts differ at queries {np.nonzero(gc != wc)[0][:5].tolist()}: got {gc[gc != wc][:5]}, want {wc[gc != wc][:5]}"
    bad = np.argwhere(gi != wi)
    assert len(bad) == 0, f"{what}: {len(bad)} indices differ, first at {bad[0].tolist()}: got {gi[tuple(bad[0])]} ({gd[tuple(bad[0])]!r}), want {wi[tuple(bad[0])]} ({wd[tuple(bad[0])]!r})"
    held = np.arange(gi.shape[1])[None, :] < wc[:, None]
    bad = np.argwhere((bits(gd) != bits(wd)) & held)
    assert len(bad) == 0, f"{what}: {len(bad)} distances differ, first at {bad[0].tolist()}: got {gd[tuple(bad[0])]!r}, want {wd[tuple(bad[0])]!r}"
    assert np.isnan(gd[~held]).all() and (gi[~held] == NONE).all(), f"{what}: the entries behind count are not 0xFFFFFFFF / NaN"


@functools.lru_cache(maxsize=None)
def inputs(s):
    """65 queries and 257 database sketches of s slots over a shared base, and the yardstick's blocks for both metrics: every
    smaller shape is a corner of these (a pair's distance depends on the pair alone)"""
    rng = np.random.default_rng(2000 + s)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    qm, qw = make_sketches(rng, 65, s, base)
    dm, dw = make_sketches(rng, 257, s, base)
    want = {metric: blocks(qm, qw, dm, dw, metric) for metric in ("jaccard", "weightedjaccard")}
    for a in (qm, qw, dm, dw, *[want[x][y] for x in want for y in want[x]]):
        a.setflags(write=False)
    return qm, qw, dm, dw, want


# ---- 1. planted shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 8, 33, 512])
def test_planted_shapes(s):
    """M: one query, a tile of 32 less one, exactly, plus one, three tiles with a tail; P: one sketch, a 64-wide tile less one,
    exactly, plus one, five tiles with a tail; S: one slot, less than a chunk of 32, a chunk and a tail, whole chunks; K: 1, a few,
    all 64 lanes (K > P included: count = the pairs that are not NaN).  A thinned product: all 25 (M, P) pairs with every metric
    and role, K walking through its values so that each meets every M, every P and every variant."""
    from hulk_amd.smash import search
    qm, qw, dm, dw, want = inputs(s)
    for metric, role in VARIANTS:
        D = want[metric][role]
        inner = int(((D > 0) & (D < 1)).sum())
        print(f"S {s} {metric} {role}: {inner} of {D.size} expected distances strictly inside (0, 1)")
        if s > 1:
            assert 3 * inner >= D.size, "the inputs are no test: too few distances strictly between 0 and 1"
        if s == 8:                                                  # the index tie-break decides the answer
            srt = np.sort(D, axis=1)
            for k in KS:
                tied = float((srt[:, k - 1] == srt[:, k]).mean())
                print(f"    K {k}: the K-th and (K+1)-th expected distances are equal in {tied:.2f} of the rows")
                # (weighted, role column: every database sketch is the subject with weights of its own, so two of them are at
                # one distance from a query only by accident — 0.02 of the rows here; the figure is printed, the condition
                # holds for the three variants in which a row shares the subject's weights)
                if (metric, role) != ("weightedjaccard", "column"):
                    assert tied >= 0.5, "the inputs are no test: the tie-break by index decides nothing"
    seen = set()
    for v, (metric, role) in enumerate(VARIANTS):
        for i, m in enumerate(MS):
            for j, p in enumerate(PS):
                k = KS[(i + 2 * j + v) % 3]
                seen.add((k, metric, role)); seen.add((k, "M", m)); seen.add((k, "P", p))
                got = search(qm[:m], qw[:m], dm[:p], dw[:p], k, metric, role)
                assert_hits(got, select(want[metric][role][:m, :p], k), f"M {m} P {p} S {s} K {k} {metric} {role}")
                if p < k:
                    assert (got[2] <= p).all()
    assert len(seen) == 3 * (4 + 5 + 5), "the thinned product leaves a combination out"


# ---- 2. strips and query blocks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [8, 33])
def test_strips_and_blocks_do_not_change_the_result(s):
    """the same inputs at M = 65, P = 257: the default scratch takes the database in one strip and the queries in one block; the
    smallest scratch that holds a tile (32 queries x 64 sketches) takes 5 strips and 3 blocks; a middle one something in between"""
    from hulk_amd.smash import search
    qm, qw, dm, dw, want = inputs(s)
    tile = 64 * (s * 32 + 32 * 8)
    for metric, role in VARIANTS:
        for k in KS:
            w = select(want[metric][role], k)
            one, many, mid = {}, {}, {}
            a = search(qm, qw, dm, dw, k, metric, role, stats=one)
            b = search(qm, qw, dm, dw, k, metric, role, scratch_bytes=tile, stats=many)
            c = search(qm, qw, dm, dw, k, metric, role, scratch_bytes=3 * tile, stats=mid)
            assert (one["strips"], one["query_blocks"]) == (1, 1), one
            assert many["strips"] >= 5 and many["query_blocks"] >= 3, many
            assert mid["strips"] > 1, mid
            for got, st in ((a, one), (b, many), (c, mid)):
                assert_hits(got, w, f"S {s} K {k} {metric} {role} {st['strips']} strips {st['query_blocks']} blocks")
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---- 3. planted values ------------------------------------------------------------------------------------------------------------
NAMES = ["A", "Aneg", "B", "C", "Cr", "D", "E"]
IX = {n: i for i, n in enumerate(NAMES)}
PLANTED_MINS = np.array([[1, 2, 3, 4],                      # A
                         [1, 2, 3, 4],                      # Aneg: A's weights with the signs turned (equal magnitude)
                         [5, 6, 7, 8],                      # B: no slot in common with A
                         [2 ** 63 + 1, 2, 3, 4],            # C and Cr: 2^63 + 1 and 2^63 are one float64
                         [2 ** 63, 2, 3, 4],
                         [1, 2, 3, 4],                      # D: MaxFloat64 weights, the union overflows
                         [1, 2, 3, 4]], dtype=np.uint64)    # E: weights -0.0 / 0.0 only, 0 / 0
PLANTED_WEIGHTS = np.array([[0.5, -0.5, 0.25, -0.25],
                            [-0.5, 0.5, -0.25, 0.25],
                            [-1e-3, -2e-3, 3e-3, -4e-3],
                            [-1e-3, -2e-3, -3e-3, -4e-3],
                            [-2e-3, -2e-3, -3e-3, -4e-3],
                            [MAXF, MAXF, MAXF, MAXF],
                            [-0.0, 0.0, -0.0, 0.0]])


def test_planted_values():
    """the seven sketches of tests/test_gpu_panel.py::test_kernel_planted_values, searched among themselves (the diagonal included).
    As a weighted subject E is 0 / 0 against everybody and D is Inf / Inf against every sketch it shares a slot with — all but B,
    where it is 0 / Inf: distance 1, a hit like any other, at the end of the list."""
    from hulk_amd.smash import search
    mins, weights = PLANTED_MINS, PLANTED_WEIGHTS
    got = {}
    for metric, role in VARIANTS:
        D = blocks(mins, weights, mins, weights, metric)[role]
        got[metric, role] = g = search(mins, weights, mins, weights, 7, metric, role)
        print(metric, role, "\n", g[0].astype(np.int64), "\n", g[1], g[2])
        assert_hits(g, select(D, 7), f"planted {metric} {role}")
        index, dist, count = g
        for a, b in (("C", "Cr"), ("Cr", "C")):                     # they find each other at distance 0, before everything that differs
            at = index[IX[a], :count[IX[a]]].tolist().index(IX[b])
            assert dist[IX[a], at] == 0 and at <= 1
    index, dist, count = got["jaccard", "row"]
    assert index[IX["A"], :4].tolist() == [IX["A"], IX["Aneg"], IX["D"], IX["E"]] and not dist[IX["A"], :4].any()
    assert (count == 7).all()
    index, dist, count = got["weightedjaccard", "row"]
    assert count[IX["E"]] == 0 and (index[IX["E"]] == NONE).all() and np.isnan(dist[IX["E"]]).all()
    assert count[IX["D"]] == 1 and index[IX["D"], 0] == IX["B"] and dist[IX["D"], 0] == 1
    assert count[IX["A"]] == 7 and index[IX["A"], :4].tolist() == [IX["A"], IX["Aneg"], IX["D"], IX["E"]], "the query's weights only: D and E are plain hits"
    index, dist, count = got["weightedjaccard", "column"]
    for q in range(7):
        hits = index[q, :count[q]].tolist()
        assert IX["E"] not in hits, "E as the subject is NaN against everybody"
        assert (IX["D"] in hits) == (q == IX["B"]), "D as the subject is NaN but against B (0 / Inf)"
        assert count[q] == (6 if q == IX["B"] else 5)


# ---- 4. max_distance --------------------------------------------------------------------------------------------------------------
def test_max_distance():
    from hulk_amd.smash import search
    qm, qw, dm, dw, want = inputs(8)
    qm, qw, dm, dw = qm.copy(), qw.copy(), dm.copy(), dw.copy()
    dm[3] = qm[0]                                                   # an exact match of query 0 ...
    dm[200] = qm[0]; dm[200, :4] = 194481 + np.arange(4)            # ... and a sketch with exactly half of its slots
    for metric, role in VARIANTS:
        D = blocks(qm, qw, dm, dw, metric)[role]
        if metric == "jaccard":
            assert D[0, 3] == 0 and D[0, 200] == 0.5
        free = select(D, 64)
        for md in (0.0, 0.5, 0.25, 1.0, -1.0, float("nan"), None):
            got = search(qm, qw, dm, dw, 64, metric, role, max_distance=md)
            want_md = select(D, 64, None if md is None or md != md else md)
            assert_hits(got, want_md, f"{metric} {role} max_distance {md}")
            index, dist, count = got
            if md == 0.0:
                assert not np.nan_to_num(dist).any() and 3 in index[0, :count[0]], "0.0 returns the exact matches and nothing else"
            if md == 0.5 and metric == "jaccard":
                assert 200 in index[0, :count[0]] and np.nanmax(dist) == 0.5, "0.5 is inclusive"
            if md is None or md != md or md in (1.0, -1.0):
                assert_hits(got, free, f"{metric} {role} max_distance {md} is no limit")


# ---- 5. self search ---------------------------------------------------------------------------------------------------------------
def test_self_search():
    from hulk_amd.smash import search
    qm, qw, _, _, _ = inputs(33)
    qw = qw.copy()
    qw[7] = 0.0                                                     # a sketch that is NaN as a weighted subject, its own diagonal included
    for metric, role in VARIANTS:
        D = blocks(qm, qw, qm, qw, metric)[role]
        for k in (1, 5, 64):
            for scratch in (0, 64 * (33 * 32 + 32 * 8)):
                got = search(qm, qw, None, None, k, metric, role, self_search=True, scratch_bytes=scratch)
                assert_hits(got, select(D, k, no_diagonal=True), f"self {metric} {role} K {k} scratch {scratch}")
                index, _, count = got
                assert not (index == np.arange(65, dtype=np.uint32)[:, None]).any(), "a sketch is its own hit"
            plain = search(qm, qw, qm, qw, k, metric, role)
            assert_hits(plain, select(D, k), f"db = queries {metric} {role} K {k}")
            diag_ok = ~np.isnan(np.diag(D))
            assert (plain[0][diag_ok, 0] == np.nonzero(diag_ok)[0]).all(), "without the flag the diagonal is hit 0 wherever it is not NaN"
            if metric == "weightedjaccard":
                assert not diag_ok[7] or role == "column"


# ---- 5b. beyond one pass of the selection -------------------------------------------------------------------------------------------
# k_search_select reads a strip's row 512 distances a pass.  Five queries against up to 1100 sketches: tests/search_inputs.py has the
# inputs and the conditions that make them a test (they run without a GPU in tests/test_search_cpu.py)
@pytest.mark.parametrize("p", si.LONG_PS)
@pytest.mark.parametrize("s,metric", si.LONG_CASES)
def test_one_strip_longer_than_one_pass(s, metric, p):
    """one strip of 511, 512, 513 (a second pass of one candidate, and that one a hit), 1023, 1024, 1025 and 1100 sketches (a third
    pass with a tail); K = 1, 2, 33, 63, 64 thinned over the strip lengths and the two roles (tests/search_inputs.py: thinned)"""
    from hulk_amd.smash import search
    qm, qw, dm, dw = si.long_inputs(s)
    ran = 0
    for role in si.ROLES:
        D = si.long_blocks(s, metric)[role]
        for k in [k for pp, k in si.thinned(role) if pp == p]:
            st = {}
            got = search(qm, qw, dm[:p], dw[:p], k, metric, role, stats=st)
            assert (st["strips"], st["query_blocks"]) == (1, 1), st
            assert_hits(got, select(D[:, :p], k), f"P {p} S {s} K {k} {metric} {role}")
            ran += 1
    assert ran == len(si.LONG_KS), "every K meets this P, under one role or the other"


@pytest.mark.parametrize("s,metric", si.LONG_CASES)
def test_two_strips_longer_than_one_pass(s, metric):
    """1100 sketches in strips of 576 and 524: the second strip starts at pbase = 576 and has a second pass with a tail of its own"""
    from hulk_amd.smash import search
    si.check_long_strips(s, metric)
    qm, qw, dm, dw = si.long_inputs(s)
    for role in si.ROLES:
        D = si.long_blocks(s, metric)[role]
        for k in si.LONG_KS:
            st = {}
            got = search(qm, qw, dm, dw, k, metric, role, scratch_bytes=si.strip_scratch(s), stats=st)
            assert st["strips"] == 2, st
            assert_hits(got, select(D, k), f"P {si.LONG_P} S {s} K {k} {metric} {role} in strips of {si.STRIP}")


@pytest.mark.parametrize("order", si.ORDERS)
@pytest.mark.parametrize("s,metric", si.LONG_CASES)
def test_database_orders_made_for_the_selection(s, metric, order):
    """P = 1100, K = 64.  descending by the distance to query 0: candidate after candidate enters at rank 0 and the tail moves up;
    ascending: nothing enters after the first K; 1100 identical sketches: every key ties and the index alone decides; copies of query
    0's nearest sketch at 509 .. 515: a run of equal distances across the border of the first pass"""
    from hulk_amd.smash import search
    qm, qw, _, _ = si.long_inputs(s)
    for role in si.ROLES:
        entered = si.check_orders(s, metric, role)[order]
        dm, dw, D = si.ordered_database(s, metric, role, order)
        print(f"S {s} {metric} {role} {order}: {entered} of {si.LONG_P} candidates enter query 0's list")
        want = select(D, si.LONG_K)
        for scratch in (0, si.strip_scratch(s)):
            got = search(qm, qw, dm, dw, si.LONG_K, metric, role, scratch_bytes=scratch)
            assert_hits(got, want, f"P {si.LONG_P} S {s} {metric} {role} database {order} scratch {scratch}")
        if order == "identical":
            assert (got[0] == np.arange(si.LONG_K, dtype=np.uint32)[None, :]).all() and (bits(got[1]) == bits(got[1])[:, :1]).all()


@pytest.mark.parametrize("s,metric", si.LONG_CASES)
def test_self_search_and_a_limit_beyond_one_pass(s, metric):
    """N = 1100 sketches among themselves: the diagonal lies in every pass, and a max_distance that leaves many queries fewer than K
    hits rejects and accepts candidates of the second and the third pass"""
    from hulk_amd.smash import search
    _, _, dm, dw = si.long_inputs(s)
    n = si.pass_length()
    for role in si.ROLES:
        lim, want, free = si.check_self_search(s, metric, role)
        got = search(dm, dw, None, None, si.LONG_K, metric, role, max_distance=lim, self_search=True)
        assert_hits(got, want, f"self N {si.LONG_P} S {s} {metric} {role} max_distance {lim!r}")
        index, _, count = got
        held = np.arange(si.LONG_K)[None, :] < count[:, None]
        assert (held & (index < n)).any() and (held & (index >= n) & (index < 2 * n)).any() and (held & (index >= 2 * n)).any(), "hits on both sides of every pass border"
        assert not (index == np.arange(si.LONG_P, dtype=np.uint32)[:, None]).any(), "a sketch is its own hit"
        assert_hits(search(dm, dw, None, None, si.LONG_K, metric, role, self_search=True), free, f"self N {si.LONG_P} S {s} {metric} {role}")


# ---- 6. the directory form and the CLI ------------------------------------------------------------------------------------------------
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


def test_directory_form_and_cli(tmp_path):
    """40 sketch files, 3 of them the queries (one with a comma in its name: encoding/csv quotes it).  search_files and the CLI write
    the same CSV, and every similarity in it is the string hulk_smash_files writes for that pair with all files in one directory."""
    from hulk_amd import smash
    rng = np.random.default_rng(66)
    S = 50
    base = rng.integers(0, 194481, size=S).astype(np.uint64)
    mins, weights = make_sketches(rng, 40, S, base)
    union, qdir, ddir = tmp_path / "union", tmp_path / "q", tmp_path / "db"
    for d in (union, qdir, ddir):
        d.mkdir()
    qnames = ["q0.json", "q,1.json", "q2.json"]
    for i in range(40):
        name = qnames[i] if i < 3 else f"s{i:02d}.json"
        for d in (union, qdir if i < 3 else ddir):
            write_sketch(str(d / name), mins[i], weights[i])
    for metric, role, k in (("jaccard", "row", 5), ("weightedjaccard", "row", 40), ("weightedjaccard", "column", 3)):
        order, _ = smash.smash(str(union), str(tmp_path / f"u_{metric}"), 21, "histosketch", metric)
        matrix = [l.split(",") for l in open(str(tmp_path / f"u_{metric}") + ".hulk-matrix.csv").read().splitlines()[1:]]
        pos = {os.path.basename(p): i for i, p in enumerate(order)}
        out = str(tmp_path / f"py_{metric}_{role}.csv")
        st = {}
        q_order, d_order, index, dist, count = smash.search_files([str(qdir / n) for n in qnames], [str(p) for p in ddir.iterdir()], k,
                                                                  metric=metric, role=role, csv_path=out, stats=st)
        assert [os.path.basename(p) for p in q_order] == sorted(qnames) and len(d_order) == 37 and st["strips"] == 1
        assert (count == min(k, 37)).all()
        lines = open(out).read().splitlines()
        assert lines[0] == "query,rank,hit,similarity" and len(lines) == 1 + int(count.sum())
        at = 1
        for i, q in enumerate(q_order):
            for j in range(count[i]):
                hit = d_order[index[i, j]]
                a, b = pos[os.path.basename(q)], pos[os.path.basename(hit)]
                sim = matrix[a][b] if role == "row" else matrix[b][a]
                assert lines[at] == f"{smash.go_csv_field(q)},{j + 1},{smash.go_csv_field(hit)},{sim}", (lines[at], sim)
                at += 1
        assert '"' + str(qdir / "q,1.json") + '"' in open(out).read()
        r = cli(["search", "-q", str(qdir), "-d", str(ddir), "-m", metric, "--role", role, "--top", str(k), "-o", str(tmp_path / "cli")])
        assert r.returncode == 0 and "HULK SEARCH!" in r.stdout, r.stdout + r.stderr
        assert open(str(tmp_path / "cli") + ".hulk-search.csv").read() == open(out).read()
    # files and directories mixed after -q, a distance limit, --self
    r = cli(["search", "-q", str(qdir / "q0.json"), str(qdir / "q2.json"), "-d", str(ddir), "--top", "4", "--maxDistance", "0.5", "-o", str(tmp_path / "two")])
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l.split(",") for l in open(str(tmp_path / "two") + ".hulk-search.csv").read().splitlines()[1:]]
    assert rows and {x[0] for x in rows} <= {str(qdir / "q0.json"), str(qdir / "q2.json")} and all(float(x[3]) >= 50.0 for x in rows)
    r = cli(["search", "-q", str(ddir), "--self", "--top", "2", "-o", str(tmp_path / "knn")])
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l.split(",") for l in open(str(tmp_path / "knn") + ".hulk-search.csv").read().splitlines()[1:]]
    assert len(rows) == 2 * 37 and all(x[0] != x[2] for x in rows)
    # MinHash signatures carry no weights: jaccard works, weightedjaccard is the reference's refusal
    for algo in ("khf", "kmv"):
        d = tmp_path / algo
        d.mkdir()
        for i in range(6):
            write_sketch(str(d / f"m{i}.json"), mins[i], None, algo=algo)
        r = cli(["search", "-q", str(d / "m0.json"), "-d", str(d), "-a", algo, "--top", "3", "-o", str(tmp_path / algo / "out")])
        assert r.returncode == 0, r.stdout + r.stderr
        rows = [l.split(",") for l in open(str(tmp_path / algo / "out") + ".hulk-search.csv").read().splitlines()[1:]]
        D = blocks(mins[:1], weights[:1], mins[:6], weights[:6], "jaccard")["row"]
        want = select(D, 3)
        assert [x[2] for x in rows] == [str(d / f"m{i}.json") for i in want[0][0]] and rows[0][3] == "100.00"
        assert [x[3] for x in rows] == [smash.go_format_f2(100 - (v * 100)) for v in want[1][0]]
        r = cli(["search", "-q", str(d / "m0.json"), "-d", str(d), "-a", algo, "-m", "weightedjaccard", "-o", str(tmp_path / algo / "w")])
        assert r.returncode == 1 and "weighted jaccard is only supported for histosketches" in r.stdout


# ---- 7. the C++ host ----------------------------------------------------------------------------------------------------------------
def test_cpp_host_matches_the_python_binding(tmp_path):
    from hulk_amd.smash import search
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    exe = str(tmp_path / "search_driver")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "search_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    s = 33
    qm, qw, dm, dw, _ = inputs(s)

    def dump(path, mins, weights):
        with open(path, "w") as fh:
            for a, b in zip(mins, weights):
                fh.write(" ".join([str(int(v)) for v in a] + [float(v).hex() for v in b]) + "\n")
    qf, df = str(tmp_path / "q.txt"), str(tmp_path / "db.txt")
    dump(qf, qm, qw); dump(df, dm, dw)
    tile = 64 * (s * 32 + 32 * 8)
    for metric, role, k, md, scratch, self_search in (("jaccard", "row", 5, -1.0, 0, False), ("weightedjaccard", "row", 64, -1.0, tile, False),
                                                      ("weightedjaccard", "column", 3, 0.9, 0, False), ("weightedjaccard", "row", 4, -1.0, 0, True)):
        r = subprocess.run([exe, qf, "-" if self_search else df, str(s), str(k), metric, role, repr(md), str(scratch)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        st = {}
        if self_search:
            index, dist, count = search(qm, qw, None, None, k, metric, role, max_distance=md, self_search=True, scratch_bytes=scratch, stats=st)
        else:
            index, dist, count = search(qm, qw, dm, dw, k, metric, role, max_distance=md, scratch_bytes=scratch, stats=st)
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 66 and lines[-1] == f"stats {st['strips']} {st['query_blocks']}"
        for i, line in enumerate(lines[:-1]):
            f = line.split()
            assert int(f[0]) == i and int(f[1]) == count[i] == len(f) - 2
            assert [int(x.split(":")[0]) for x in f[2:]] == index[i, :count[i]].tolist()
            assert [float.fromhex(x.split(":")[1]) for x in f[2:]] == dist[i, :count[i]].tolist()
