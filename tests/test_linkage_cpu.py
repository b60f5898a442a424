"""Complete-, average- and single-linkage dendrograms (hulk_linkage, hulk_linkage_files), the parts that need no GPU: the header
declares the entry points and the built library exports them, every argument error is refused with its text before the library looks
for a device, the Python binding and the CLI refuse an unknown linkage, the inputs of tests/test_gpu_linkage.py test what they claim
(tests/linkage_inputs.py, evaluated against oracle.pyorc), the yardstick is right on a hand-worked example and agrees with
scipy.cluster.hierarchy.linkage where SciPy is installed, and the C++ driver compiles and links."""
import ctypes
import io
import os
import re
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

import linkage_inputs as li
from conftest import ROOT

ENTRY_POINTS = ("hulk_linkage", "hulk_linkage_files")
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
    assert "typedef struct hulk_linkage_opts" in code and "typedef struct hulk_linkage_stats" in code
    assert "#define HULK_ABI_VERSION 4" in hdr, "additions only: the ABI version stays"
    defs = dict(re.findall(r"#define (HULK_LINKAGE_\w+) (\d+)u?\b", code))
    assert (int(defs["HULK_LINKAGE_SINGLE"]), int(defs["HULK_LINKAGE_COMPLETE"]), int(defs["HULK_LINKAGE_AVERAGE"])) == (0, 1, 2)
    assert (_lib.HULK_LINKAGE_SINGLE, _lib.HULK_LINKAGE_COMPLETE, _lib.HULK_LINKAGE_AVERAGE) == (0, 1, 2)
    assert int(defs["HULK_LINKAGE_MAX_N"]) == _lib.HULK_LINKAGE_MAX_N == 65536
    # the structs as the header lays them out
    assert ctypes.sizeof(_lib.LinkageOpts) == 48 and _lib.LinkageOpts.method.offset == 4 and _lib.LinkageOpts.flags.offset == 8
    assert _lib.LinkageOpts.reserved.offset == 16
    assert ctypes.sizeof(_lib.LinkageStats) == 40 and _lib.LinkageStats.merges.offset == 24 and _lib.LinkageStats.rows_rescanned.offset == 32
    if os.path.exists(_lib.EXP_LIB_PATH):
        X = ctypes.CDLL(_lib.EXP_LIB_PATH)
        assert all(hasattr(X, n) for n in ENTRY_POINTS)
    mk = open(os.path.join(ROOT, "hulk_amd", "csrc", "Makefile")).read()
    assert "hulk_linkage.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1), "the unit is part of the build and of the source hash"


def _call(L, _lib, *, metric=0, method=1, flags=0, reserved=(0, 0, 0, 0), n=3, S=4, mins=True, weights=True, a=True, b=True, d=True, size=True,
          nm=True, opts=True, tiny=False):
    rows = 1 if tiny else max(n, 1)                                 # (tiny: the arrays of a refused call are never touched)
    m = np.arange(rows * max(S, 1), dtype=np.uint64); w = np.ones(rows * max(S, 1))
    ea = np.zeros(rows, dtype=np.uint32); eb = np.zeros(rows, dtype=np.uint32); ed = np.zeros(rows); es = np.zeros(rows, dtype=np.uint32)
    count = ctypes.c_uint32(77)
    o = _lib.LinkageOpts(metric=metric, method=method, flags=flags)
    for i, v in enumerate(reserved):
        o.reserved[i] = v
    rc = L.hulk_linkage(0, m.ctypes.data if mins else None, w.ctypes.data if weights else None, n, S, ctypes.byref(o) if opts else None,
                        ea.ctypes.data if a else None, eb.ctypes.data if b else None, ed.ctypes.data if d else None,
                        es.ctypes.data if size else None, ctypes.addressof(count) if nm else None, None)
    return rc, L.hulk_last_error(None).decode()


def test_every_argument_error_is_refused_with_its_text_before_a_device_is_looked_for():
    """each of these returns HULK_ERR_ARG, not HULK_ERR_NO_DEVICE: without a device too, the argument checks come first"""
    from hulk_amd import _lib
    L = _lib.load()
    cases = [
        (dict(mins=False), "hulk_linkage: NULL"),
        (dict(weights=False), "hulk_linkage: NULL"),
        (dict(a=False), "hulk_linkage: NULL"),
        (dict(b=False), "hulk_linkage: NULL"),
        (dict(d=False), "hulk_linkage: NULL"),
        (dict(size=False), "hulk_linkage: NULL"),
        (dict(nm=False), "hulk_linkage: NULL"),
        (dict(opts=False), "hulk_linkage: NULL"),
        (dict(n=0), "n and sketch_size must be positive"),
        (dict(S=0), "n and sketch_size must be positive"),
        (dict(n=_lib.HULK_LINKAGE_MAX_N + 1, S=1, tiny=True), "n must be at most 65536"),
        (dict(n=2 ** 32 - 1, S=1, tiny=True), "n must be at most 65536"),
        (dict(metric=2), "hulk_linkage: metric"),
        (dict(metric=-1), "hulk_linkage: metric"),
        (dict(method=3), "hulk_linkage: method"),
        (dict(method=-1), "hulk_linkage: method"),
        (dict(metric=3, S=_lib.HULK_MINHASH_MAX_SKETCH + 1, n=1), "bottomk takes a sketch_size of at most 4096"),
        (dict(flags=1), "unknown flags"),
        (dict(reserved=(0, 0, 0, 1)), "reserved fields must be zero"),
        (dict(reserved=(7, 0, 0, 0)), "reserved fields must be zero"),
    ]
    for kw, text in cases:
        rc, msg = _call(L, _lib, **kw)
        assert rc == ERR_ARG and text in msg, (kw, rc, msg)
    # what is valid gets past the argument checks (and then finds no device, or runs)
    for kw in (dict(), dict(n=1), dict(method=0), dict(method=2), dict(metric=1), dict(metric=3, weights=False)):
        rc, msg = _call(L, _lib, **kw)
        assert rc in (0, ERR_NO_DEVICE), (kw, rc, msg)


def test_python_binding_refuses_bad_arguments():
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    rng = np.random.default_rng(1)
    m = rng.integers(0, 100, size=(3, 8)).astype(np.uint64); w = -rng.random((3, 8))
    with pytest.raises(HulkError, match="supplied linkage is not available: ward") as ei:
        smash.linkage(m, w, "ward")
    assert ei.value.code == ERR_ARG
    with pytest.raises(HulkError, match="supplied distance metric is not available: cosine"):
        smash.linkage(m, w, "complete", metric="cosine")
    with pytest.raises(ValueError):
        smash.linkage(m, w[:, :7], "complete")
    with pytest.raises(HulkError, match="supplied linkage is not available: ward"):
        smash.linkage_files(["a.json"], "ward")
    with pytest.raises(HulkError, match="supplied algorithm not available: minhash"):
        smash.linkage_files(["a.json"], "complete", algo="minhash")
    for cut in (-0.1, 1.5, float("inf")):
        with pytest.raises(HulkError, match=r"cut_distance must be in \[0, 1\]"):
            smash.linkage_files(["a.json"], "complete", cut_distance=cut, cut_csv_path="x.csv")
    with pytest.raises(HulkError, match="a cut_distance without a cut_csv_path"):
        smash.linkage_files(["a.json"], "average", cut_distance=0.5)
    with pytest.raises(HulkError) as ei:
        smash.linkage_files([], "complete")
    assert ei.value.code == ERR_ARG and ei.value.message == "no sketch files supplied\n"
    # the library's own refusal of a method name it does not know
    L = smash._lib.load()
    err = ctypes.create_string_buffer(4096)
    arr = (ctypes.c_char_p * 1)(b"a.json")
    rc = L.hulk_linkage_files(0, arr, 1, 21, b"histosketch", b"jaccard", b"ward", 0, None, float("nan"), None, None, None, None, None, None, None, err, len(err))
    assert rc == ERR_ARG and b"supplied linkage is not available: ward\nplease select one of the following: [single complete average]" in err.value


def _sketch_files(tmp_path, n, S, seed=3):
    from hulk_amd.sketchio import HULKdata, HistoSketch
    rng = np.random.default_rng(seed)
    for i in range(n):
        d = HULKdata()
        d.filename, d.banner_label = "reads.fq,", "blank"
        d.add(HistoSketch(21, rng.integers(0, 21 ** 4, size=S, dtype=np.uint64), -rng.random(S), 21 ** 4, False))
        d.write_json(str(tmp_path / f"d{i:02d}.json"))


def test_cli_refuses_an_unknown_linkage(tmp_path):
    from hulk_amd.__main__ import main
    db = tmp_path / "db"
    db.mkdir()
    _sketch_files(db, 2, 8)
    out = str(tmp_path / "out")
    for extra, text in ((["--linkage", "ward"], "supplied linkage is not available: ward\nplease select one of the following: ['single', 'complete', 'average']"),
                        (["--linkage", "complete", "--cut", "1.5"], "--cut must be between 0 and 1"),
                        (["--linkage", "average", "-m", "cosine"], "supplied distance metric is not available: cosine")):
        buf = io.StringIO()
        with redirect_stdout(buf):
            rc = main(["dendrogram", "-d", str(db), "-o", out] + extra)
        assert rc == 1, (extra, buf.getvalue())
        assert "ERROR---> " + text in buf.getvalue(), buf.getvalue()
        assert sorted(os.listdir(tmp_path)) == ["db"], "nothing is written"


def test_the_yardstick_on_a_hand_worked_example_with_ties():
    nan = float("nan")
    # W: (0,1) 0.5 (one direction NaN); (0,2) 0.25; (1,2) 0.25 (the other direction 0.75); (0,3) 0.5 (the other direction 0.9);
    # (1,3) 0.5; (2,3) 0.5; 4 has no distance to anything
    D = np.array([[0.0, 0.50, 0.25, 0.50, nan],
                  [nan, 0.0, 0.75, nan, nan],
                  [0.25, 0.25, 0.0, 0.50, nan],
                  [0.90, 0.50, 0.50, 0.0, nan],
                  [nan, nan, nan, nan, nan]])
    # (0,2) first (the smaller pair of the two at 0.25); then d(0,1) = min / max / mean of 0.5 and 0.25
    a, b, d, s = li.agglomerate(D, "single")
    assert (a.tolist(), b.tolist(), d.tolist(), s.tolist()) == ([0, 0, 0], [2, 1, 3], [0.25, 0.25, 0.5], [2, 3, 4])
    a, b, d, s = li.agglomerate(D, "complete")
    assert (a.tolist(), b.tolist(), d.tolist(), s.tolist()) == ([0, 0, 0], [2, 1, 3], [0.25, 0.5, 0.5], [2, 3, 4])
    a, b, d, s = li.agglomerate(D, "average")
    assert (a.tolist(), b.tolist(), d.tolist(), s.tolist()) == ([0, 0, 0], [2, 1, 3], [0.25, 0.375, 0.5], [2, 3, 4])
    # all ties: the key's order decides — a star at 0; a pair at +inf never merges, and under complete linkage neither do the clusters
    for method in li.METHODS:
        a, b, d, s = li.agglomerate(np.full((6, 6), 0.5), method)
        assert a.tolist() == [0] * 5 and b.tolist() == [1, 2, 3, 4, 5] and s.tolist() == [2, 3, 4, 5, 6]
        assert [len(x) for x in li.agglomerate(np.zeros((1, 1)), method)] == [0] * 4
        assert [len(x) for x in li.agglomerate(np.full((3, 3), nan), method)] == [0] * 4
    X = np.array([[0.0, 0.1, nan], [0.1, 0.0, 0.2], [nan, 0.2, 0.0]])
    assert li.agglomerate(X, "single")[1].tolist() == [1, 2] and li.agglomerate(X, "single")[2].tolist() == [0.1, 0.2]
    assert li.agglomerate(X, "complete")[1].tolist() == [1] and li.agglomerate(X, "average")[1].tolist() == [1]
    # average: the sizes weigh — {0, 1} (at 0.1) to 2: (1 * 0.4 + 1 * 0.8) / 2; then {0, 1, 2} to 3: (2 * d({0,1},3) + 1 * d(2,3)) / 3
    Y = np.array([[0.0, 0.1, 0.4, 0.9], [0.1, 0.0, 0.8, 0.7], [0.4, 0.8, 0.0, 1.0], [0.9, 0.7, 1.0, 0.0]])
    a, b, d, s = li.agglomerate(Y, "average")
    d03 = (1.0 * 0.9 + 1.0 * 0.7) / 2.0
    assert d.tolist() == [0.1, (1.0 * 0.4 + 1.0 * 0.8) / 2.0, (2.0 * d03 + 1.0 * 1.0) / 3.0] and s.tolist() == [2, 3, 4]


def test_the_inputs_are_a_test():
    li.check_ties()
    tau = li.check_complete_differs_from_single()
    print("complete and single linkage differ at", tau)
    print("clusters left on the weighted forest set:", li.check_weighted_forest())
    li.check_stars()
    # single linkage: the heights are the minimum spanning forest's, and every cut is the threshold clustering
    import cluster_inputs as ci
    import dendrogram_inputs as di
    for kind, arg, metric in (("planted_chains", 8, "jaccard"), ("random_set", 33, "weightedjaccard"), ("random_set", 1, "jaccard"),
                              ("weighted_set", None, "weightedjaccard")):
        a, b, d, s = li.reference(kind, arg, metric, "single")
        assert np.array_equal(np.sort(li.bits(d)), np.sort(li.bits(di.reference(kind, arg, metric)[2]))), (kind, arg, metric)
        assert (np.diff(d) >= 0).all()
        D = li.named_set(kind, arg, metric)[2]
        for tau in (0.0, 0.25, 0.5, ci.chain_tau(33), 1.0):
            assert np.array_equal(di.cut_labels(len(D), a, b, d, tau), ci.components(D, tau)[0]), (kind, arg, metric, tau)
    # complete linkage: heights never step down, and each is the largest W inside the cluster it creates
    for kind, arg, metric in (("random_set", 8, "jaccard"), ("random_set", 33, "weightedjaccard")):
        a, b, d, s = li.reference(kind, arg, metric, "complete")
        assert (np.diff(d) >= 0).all()
        W = li.weights_matrix(li.named_set(kind, arg, metric)[2])
        for members, h, size in zip(li.member_sets(257, a, b), d, s):
            m = sorted(members)
            assert len(m) == size and h == max(W[i, j] for i in m for j in m if i < j)
    # the grid set is above one workgroup's lanes
    assert li.GRID_N > 1024 and len(li.grid_set()[0]) == li.GRID_N


def test_linkage_matrix_and_cut_dendrogram_read_the_merges():
    from hulk_amd.smash import cut_dendrogram, linkage_matrix
    a, b, d, s = li.reference("random_set", 33, "weightedjaccard", "average")
    Z = linkage_matrix(257, a, b, d)
    assert Z.shape == (256, 4) and np.array_equal(Z[:, 2], d) and np.array_equal(Z[:, 3], s) and (Z[:, 0] < Z[:, 1]).all()
    labels, k = cut_dendrogram(257, a, b, d, float(np.median(d)))
    assert 1 < k < 257 and labels.dtype == np.uint32


def test_the_yardstick_against_scipy_if_it_is_there():
    """a tie-free symmetric input of N = 64: under complete linkage the heights are equal as bits and the member sets per merge are
    the same; under average linkage the member sets are the same and the heights agree within rtol 1e-12 (SciPy's nearest-neighbour
    chain applies the same update in another order: at most 3 roundings per update over at most 63 levels, about 2e-14)"""
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    mins, weights, D = li.tie_free_set()
    n = len(D)
    W = li.weights_matrix(D).copy()
    np.fill_diagonal(W, 0.0)
    for method in ("complete", "average"):
        a, b, d, s = li.agglomerate(D, method)
        assert len(a) == n - 1
        Z = hierarchy.linkage(squareform(W, checks=False), method=method)
        ids = {i: frozenset([i]) for i in range(n)}
        theirs = []
        for t, row in enumerate(Z):
            ids[n + t] = ids[int(row[0])] | ids[int(row[1])]
            theirs.append(ids[n + t])
        ours = li.member_sets(n, a, b)
        # both orders are ascending in height; without ties the same set of clusters is created
        assert set(ours) == set(theirs), method
        by_members = {m: h for m, h in zip(theirs, Z[:, 2])}
        want = np.array([by_members[m] for m in ours])
        if method == "complete":
            assert np.array_equal(li.bits(d), li.bits(want))
        else:
            assert np.allclose(d, want, rtol=1e-12, atol=0.0)
        assert [len(m) for m in ours] == s.tolist() == [int(Z[theirs.index(m), 3]) for m in ours]


def test_cpp_linkage_driver_compiles_and_links(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "linkage_driver.cpp"), "-o", str(tmp_path / "linkage_driver"),
           "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
