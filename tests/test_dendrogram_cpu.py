"""The single-linkage dendrogram (hulk_dendrogram, hulk_dendrogram_files), the parts that need no GPU: the header declares the entry
points and the built library exports them, every argument error is refused with its text before the library looks for a device,
the Python binding and the CLI refuse bad flags, the yardstick's Kruskal is right on a hand-worked example with ties, the inputs
of tests/test_gpu_dendrogram.py test what they claim (tests/dendrogram_inputs.py, evaluated against oracle.pyorc), cut_dendrogram
and linkage_matrix read the yardstick's edges, and the host contraction (hulk_amd/csrc/hulk_boruvka.h) agrees with a sequential
Kruskal in a stand-alone program under -fsanitize=address,undefined."""
import ctypes
import io
import os
import re
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

import cluster_inputs as ci
import dendrogram_inputs as di
from conftest import ROOT

ENTRY_POINTS = ("hulk_dendrogram", "hulk_dendrogram_files")
ERR_ARG, ERR_NO_DEVICE = -30, -32


def test_header_declares_and_library_exports_the_entry_points():
    from hulk_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hulk_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(int device" % name, code), f"{name} is not declared in hulk_hip.h"
        assert hasattr(L, name), f"libhulkhip.so does not export {name}"
        assert name in _lib.ABI_SYMBOLS
    assert "typedef struct hulk_dendrogram_opts" in code and "typedef struct hulk_dendrogram_stats" in code
    assert "#define HULK_ABI_VERSION 4" in hdr, "additions only: the ABI version stays"
    L.hulk_abi_version.restype = ctypes.c_int
    assert L.hulk_abi_version() == 4
    # the structs as the header lays them out
    assert ctypes.sizeof(_lib.DendrogramOpts) == 48 and _lib.DendrogramOpts.band_rows.offset == 4 and _lib.DendrogramOpts.flags.offset == 8
    assert _lib.DendrogramOpts.reserved.offset == 16
    assert ctypes.sizeof(_lib.DendrogramStats) == 40 and _lib.DendrogramStats.rounds.offset == 24 and _lib.DendrogramStats.components.offset == 36
    if os.path.exists(_lib.EXP_LIB_PATH):
        X = ctypes.CDLL(_lib.EXP_LIB_PATH)
        assert all(hasattr(X, n) for n in ENTRY_POINTS)
    csrc = os.path.join(ROOT, "hulk_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "hulk_dendrogram.hip" in mk and "hulk_boruvka.h" in mk, "the unit and its header are part of the build and of the source hash"


def _call(L, _lib, *, metric=0, band=0, flags=0, reserved=(0, 0, 0, 0), n=3, S=4, mins=True, weights=True, a=True, b=True, d=True, ne=True,
          opts=True, tiny=False):
    size = 1 if tiny else max(n, 1)                                 # (tiny: the arrays of a refused call are never touched)
    m = np.arange(size * max(S, 1), dtype=np.uint64); w = np.ones(size * max(S, 1))
    ea = np.zeros(size, dtype=np.uint32); eb = np.zeros(size, dtype=np.uint32); ed = np.zeros(size)
    count = ctypes.c_uint32(77)
    o = _lib.DendrogramOpts(metric=metric, band_rows=band, flags=flags)
    for i, v in enumerate(reserved):
        o.reserved[i] = v
    rc = L.hulk_dendrogram(0, m.ctypes.data if mins else None, w.ctypes.data if weights else None, n, S, ctypes.byref(o) if opts else None,
                           ea.ctypes.data if a else None, eb.ctypes.data if b else None, ed.ctypes.data if d else None,
                           ctypes.addressof(count) if ne else None, None)
    return rc, L.hulk_last_error(None).decode()


def test_every_argument_error_is_refused_with_its_text_before_a_device_is_looked_for():
    """each of these returns HULK_ERR_ARG, not HULK_ERR_NO_DEVICE: without a device too, the argument checks come first"""
    from hulk_amd import _lib
    L = _lib.load()
    cases = [
        (dict(mins=False), "hulk_dendrogram: NULL"),
        (dict(weights=False), "hulk_dendrogram: NULL"),
        (dict(a=False), "hulk_dendrogram: NULL"),
        (dict(b=False), "hulk_dendrogram: NULL"),
        (dict(d=False), "hulk_dendrogram: NULL"),
        (dict(ne=False), "hulk_dendrogram: NULL"),
        (dict(opts=False), "hulk_dendrogram: NULL"),
        (dict(n=0), "n and sketch_size must be positive"),
        (dict(S=0), "n and sketch_size must be positive"),
        (dict(n=_lib.HULK_CLUSTER_MAX_N + 1, S=1), "n must be at most 2097088"),
        (dict(n=2 ** 32 - 1, S=1, tiny=True), "n must be at most 2097088"),
        (dict(metric=2), "hulk_dendrogram: metric"),
        (dict(metric=-1), "hulk_dendrogram: metric"),
        (dict(band=1), "band_rows must be a multiple of 32"),
        (dict(band=48), "band_rows must be a multiple of 32"),
        (dict(flags=1), "unknown flags"),
        (dict(reserved=(0, 0, 0, 1)), "reserved fields must be zero"),
        (dict(reserved=(7, 0, 0, 0)), "reserved fields must be zero"),
    ]
    for kw, text in cases:
        rc, msg = _call(L, _lib, **kw)
        assert rc == ERR_ARG and text in msg, (kw, rc, msg)
    # what is valid gets past the argument checks (and then finds no device, or runs)
    for kw in (dict(), dict(n=1), dict(band=32), dict(band=96), dict(metric=1)):
        rc, msg = _call(L, _lib, **kw)
        assert rc in (0, ERR_NO_DEVICE), (kw, rc, msg)


def test_python_binding_refuses_bad_arguments():
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    rng = np.random.default_rng(1)
    m = rng.integers(0, 100, size=(3, 8)).astype(np.uint64); w = -rng.random((3, 8))
    with pytest.raises(HulkError, match="band_rows must be a multiple of 32") as ei:
        smash.dendrogram(m, w, band_rows=33)
    assert ei.value.code == ERR_ARG
    with pytest.raises(HulkError, match="supplied distance metric is not available: cosine"):
        smash.dendrogram(m, w, metric="cosine")
    with pytest.raises(ValueError):
        smash.dendrogram(m, w[:, :7])
    with pytest.raises(ValueError):
        smash.dendrogram(m, w, band_rows=-32)
    with pytest.raises(HulkError, match="supplied algorithm not available: minhash"):
        smash.dendrogram_files(["a.json"], algo="minhash")
    with pytest.raises(HulkError, match="supplied distance metric is not available: cosine"):
        smash.dendrogram_files(["a.json"], metric="cosine")
    for cut in (-0.1, 1.5, float("inf")):
        with pytest.raises(HulkError, match=r"cut_distance must be in \[0, 1\]"):
            smash.dendrogram_files(["a.json"], cut_distance=cut, cut_csv_path="x.csv")
    with pytest.raises(HulkError, match="a cut_distance without a cut_csv_path"):
        smash.dendrogram_files(["a.json"], cut_distance=0.5)
    with pytest.raises(HulkError) as ei:
        smash.dendrogram_files([])
    assert ei.value.code == ERR_ARG and ei.value.message == "no sketch files supplied\n"


def _write(path, mins, weights, k=21):
    from hulk_amd.sketchio import HULKdata, HistoSketch
    d = HULKdata()
    d.filename, d.banner_label = "reads.fq,", "blank"
    d.add(HistoSketch(k, np.asarray(mins, dtype=np.uint64), np.asarray(weights, dtype=np.float64), k ** 4, False))
    d.write_json(path)


def _sketch_files(tmp_path, n, S, seed=3, prefix="d"):
    rng = np.random.default_rng(seed)
    files = []
    for i in range(n):
        p = str(tmp_path / f"{prefix}{i:02d}.json")
        _write(p, rng.integers(0, 21 ** 4, size=S, dtype=np.uint64), -rng.random(S))
        files.append(p)
    return files


def test_directory_form_reports_the_reference_texts(tmp_path):
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    db = _sketch_files(tmp_path, 3, 16)
    for files in (db, db[:1]):                                      # a set of one sketch is valid: without a device loading is all that can succeed
        try:
            smash.dendrogram_files(files)
        except HulkError as e:
            assert e.code == ERR_NO_DEVICE, (e.code, e.message)
    short = _sketch_files(tmp_path, 1, 12, seed=5, prefix="s")
    with pytest.raises(HulkError) as ei:
        smash.dendrogram_files(db + short)
    assert ei.value.message == "sketch length mismatch: 16 vs 12\n"
    with pytest.raises(HulkError, match=r"specified k-mer size \(15\) not found"):
        smash.dendrogram_files(db, ksize=15)
    with pytest.raises(HulkError, match="no sketches were produced using the kmv algorithm"):
        smash.dendrogram_files(db, algo="kmv")


def test_cli_refuses_bad_flags(tmp_path):
    from hulk_amd.__main__ import main
    db = tmp_path / "db"
    db.mkdir()
    _sketch_files(db, 2, 8)
    out = str(tmp_path / "out")
    cases = ((["--cut", "0.1", "--cutSimilarity", "90"], "at most one of --cut and --cutSimilarity may be given"),
             (["--cut", "1.5"], "--cut must be between 0 and 1"),
             (["--cut", "-0.5"], "--cut must be between 0 and 1"),
             (["--cut", "nan"], "--cut must be between 0 and 1"),
             (["--cutSimilarity", "101"], "--cutSimilarity must be between 0 and 100"),
             (["--cutSimilarity", "-1"], "--cutSimilarity must be between 0 and 100"),
             (["-m", "cosine"], "supplied distance metric is not available: cosine"),
             (["-a", "minhash"], "supplied algorithm not available: minhash\nplease select one of the following: ['histosketch', 'kmv', 'khf']"))
    for extra, text in cases:
        buf = io.StringIO()
        with redirect_stdout(buf):
            rc = main(["dendrogram", "-d", str(db), "-o", out] + extra)
        assert rc == 1, (extra, buf.getvalue())
        assert "ERROR---> " + text in buf.getvalue(), buf.getvalue()
        assert sorted(os.listdir(tmp_path)) == ["db"], "nothing is written"
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main(["dendrogram", "-o", out])
    assert rc == 1 and "no sketch directory supplied (-d)" in buf.getvalue()


def test_the_yardsticks_kruskal_on_a_hand_worked_example_with_ties():
    nan = float("nan")
    # W = fmin(D, D.T): (0,1) 0.5 one way only; (0,2) 0.25; (1,2) 0.25 (the other direction 0.75); (2,3) 0.5; (0,3), (1,3) 0.5 / NaN;
    # 4 has no distance to anything.  Sorted by (W, i, j): (0,2) (1,2) | (0,1) (0,3) (1,3) (2,3): Kruskal keeps (0,2), (1,2), (0,3)
    D = np.array([[0.0, 0.50, 0.25, 0.50, nan],
                  [nan, 0.0, 0.75, nan, nan],
                  [0.25, 0.25, 0.0, 0.50, nan],
                  [0.90, 0.50, 0.50, 0.0, nan],
                  [nan, nan, nan, nan, nan]])
    a, b, d = di.kruskal(D)
    assert a.tolist() == [0, 1, 0] and b.tolist() == [2, 2, 3] and d.tolist() == [0.25, 0.25, 0.5]
    oa, ob, od, rounds = di.offer_rounds(D)
    assert di.same_edges((oa, ob, od), (a, b, d)) and rounds == 2, "one productive pass (everything ties into 0's tree), one empty pass for the loner"
    assert di.cut_labels(5, a, b, d, 0.25).tolist() == [0, 0, 0, 3, 4] and di.cut_labels(5, a, b, d, 0.5).tolist() == [0, 0, 0, 0, 4]
    for tau in (0.0, 0.25, 0.3, 0.5, 1.0):
        assert np.array_equal(di.cut_labels(5, a, b, d, tau), ci.components(D, tau)[0])
    # all ties: the order (i, j) decides — a star at 0
    a, b, d = di.kruskal(np.full((6, 6), 0.5))
    assert a.tolist() == [0] * 5 and b.tolist() == [1, 2, 3, 4, 5] and di.offer_rounds(np.full((6, 6), 0.5))[3] == 1
    assert [len(x) for x in di.kruskal(np.zeros((1, 1)))] == [0, 0, 0] and di.offer_rounds(np.zeros((1, 1)))[3] == 0
    assert [len(x) for x in di.kruskal(np.full((3, 3), nan))] == [0, 0, 0] and di.offer_rounds(np.full((3, 3), nan))[3] == 1
    assert [di.round_bound(n) for n in (1, 2, 3, 64, 65, 257)] == [0, 2, 3, 7, 8, 10]


def test_the_inputs_are_a_test():
    rounds = di.check_multi_round()
    print(rounds)
    di.check_weighted_facts()
    di.check_ties()
    # the offer form is Kruskal on every other set too, in 1 - 2 rounds on the random ones
    for s in (8, 33):
        for metric in di.METRICS:
            assert 1 <= di.reference_rounds("random_set", s, metric) <= 2
    for order in ("ascending", "descending"):
        di.reference_rounds("ordered_chain", order, "jaccard")
    assert di.reference_rounds("weighted_set", None, "weightedjaccard") >= 1
    # stars: identical sketches at 0, disjoint ones at 1, both on sketch 0
    from oracle import pyorc
    for (mins, weights), h in ((di.identical_set(), 0.0), (di.disjoint_set(), 1.0)):
        for metric in di.METRICS:
            a, b, d = di.kruskal(pyorc.smash_matrix(mins, weights, metric))
            assert not a.any() and b.tolist() == list(range(1, 65)) and (d == h).all(), di.NO_TEST + "not a star at sketch 0"
    mins, weights = di.zero_weight_set()
    assert np.isnan(pyorc.smash_matrix(mins, weights, "weightedjaccard")).all(), di.NO_TEST + "all-zero weights do not give NaN everywhere"


def test_the_cut_of_the_yardsticks_tree_is_the_yardsticks_clustering():
    from hulk_amd.smash import cut_dendrogram
    for kind, arg, metric in (("random_set", 33, "jaccard"), ("random_set", 33, "weightedjaccard"), ("planted_chains", 8, "jaccard"),
                              ("ordered_chain", "random", "jaccard"), ("weighted_set", None, "weightedjaccard")):
        D = di.named_set(kind, arg, metric)[2]
        n = len(D)
        a, b, d = di.reference(kind, arg, metric)
        taus = [0.0, 0.5, 1.0, ci.chain_tau(8), np.nextafter(ci.chain_tau(8), 0.0), ci.chain_tau(33), np.nextafter(ci.chain_tau(33), 0.0)]
        if kind == "random_set":
            taus += ci.random_set(arg)[2][metric][1]
        for tau in taus:
            want = ci.components(D, tau)
            labels, n_clusters = cut_dendrogram(n, a, b, d, tau)
            assert labels.dtype == np.uint32 and np.array_equal(labels, want[0]) and n_clusters == want[2], (kind, arg, metric, tau)
    assert cut_dendrogram(1, [], [], [], 0.5)[0].tolist() == [0]
    with pytest.raises(ValueError):
        cut_dendrogram(3, [0], [3], [0.1], 0.5)


def test_linkage_matrix():
    from hulk_amd.smash import linkage_matrix
    # hand-worked: 0 - 2 and 1 - 3 at 0.25, joined by (2, 3) at 0.5; then 4
    Z = linkage_matrix(5, [0, 1, 2, 0], [2, 3, 3, 4], [0.25, 0.25, 0.5, 0.75])
    assert Z.tolist() == [[0, 2, 0.25, 2], [1, 3, 0.25, 2], [5, 6, 0.5, 4], [4, 7, 0.75, 5]]
    assert linkage_matrix(1, [], [], []).shape == (0, 4)
    with pytest.raises(ValueError, match="not one tree"):
        linkage_matrix(5, [0, 1, 2], [2, 3, 3], [0.25, 0.25, 0.5])       # a forest
    with pytest.raises(ValueError, match="not one tree"):
        linkage_matrix(3, [0, 0], [1, 1], [0.25, 0.5])                    # n - 1 edges that do not join n sketches
    a, b, d = di.reference("random_set", 33, "weightedjaccard")
    Z = linkage_matrix(257, a, b, d)
    assert Z.shape == (256, 4) and np.array_equal(Z[:, 2], d) and Z[-1, 3] == 257 and (Z[:, 0] < Z[:, 1]).all()
    assert sorted(Z[:, :2].astype(int).ravel().tolist()) == list(range(2 * 257 - 2)), "every sketch and every cluster but the last merges once"
    mins, weights, D = ci.weighted_set()
    a, b, d = di.kruskal(D[:40, :40])                                    # (without Z: still one tree) and a forest: the zero-weight set
    assert linkage_matrix(40, a, b, d).shape == (39, 4)
    with pytest.raises(ValueError):
        linkage_matrix(3, *di.kruskal(np.full((3, 3), np.nan)))


def test_sorted_heights_against_scipy_if_it_is_there():
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    for kind, arg, metric in (("random_set", 33, "jaccard"), ("random_set", 33, "weightedjaccard"), ("planted_chains", 8, "jaccard")):
        W = di.edge_weights(di.named_set(kind, arg, metric)[2]).copy()
        np.fill_diagonal(W, 0.0)
        assert not np.isnan(W).any()
        Z = hierarchy.linkage(squareform(W, checks=False), method="single")
        assert np.array_equal(np.sort(Z[:, 2]), di.reference(kind, arg, metric)[2])


def test_the_host_contraction_against_kruskal_under_sanitizers(tmp_path):
    """hulk_boruvka.h is HIP-free: the text hulk_dendrogram runs behind every round, in a stand-alone program that produces the
    offers with a plain loop from dense matrices (heavy ties, NaN blocks, stars, paths) and compares with a sequential Kruskal"""
    exe = str(tmp_path / "boruvka_host")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan",      # (the runtimes inside the program: it is whole on its own)
                        "-I", os.path.join(ROOT, "hulk_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "boruvka_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stdout.count(": ok") == 18, r.stdout + r.stderr[-3000:]


def test_cpp_dendrogram_driver_compiles_and_links(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "dendrogram_driver.cpp"), "-o", str(tmp_path / "dendrogram_driver"),
           "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
