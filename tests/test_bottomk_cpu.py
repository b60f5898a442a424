"""The bottom-k metric (HULK_METRIC_BOTTOMK), the parts that need no GPU: the header, the library and the bindings carry the constant;
metric 3 passes the argument checks of the five array entry points (and 2 stays refused); the *_files forms and the CLI take
"bottomk" with kmv sketches and refuse it for the others with their text; the panel keeps refusing it; the yardstick
(tests/bottomk_inputs.py) is KMVsketch.GetSimilarity and its planted inputs are what they claim; the arithmetic of the kernels
(hulk_amd/csrc/hulk_bottomk_merge.h) compiled for the host agrees with kmv.go's loop under -fsanitize=address,undefined."""
import ctypes
import io
import os
import re
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

import bottomk_inputs as bi
from conftest import ROOT

ERR_ARG, ERR_NO_DEVICE = -30, -32
BOTTOMK = 3


def test_header_library_and_bindings_carry_the_constant():
    from hulk_amd import _lib, smash
    hdr = open(os.path.join(ROOT, "include", "hulk_hip.h")).read()
    assert re.search(r"^#define HULK_METRIC_BOTTOMK 3\b", hdr, re.M) and _lib.HULK_METRIC_BOTTOMK == BOTTOMK
    assert re.search(r"^#define HULK_METRIC_JACCARD 0\b", hdr, re.M) and re.search(r"^#define HULK_METRIC_WEIGHTED_JACCARD 1\b", hdr, re.M)
    assert "#define HULK_ABI_VERSION 4" in hdr, "additions only: the ABI version stays"
    assert smash.AVAIL_METRICS == ["jaccard", "weightedjaccard", "bottomk"]
    hpp = open(os.path.join(ROOT, "include", "hulk.hpp")).read()
    assert 'if (metric == "bottomk") return HULK_METRIC_BOTTOMK;' in hpp
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "bottomk" in open(os.path.join(ROOT, doc)).read(), doc
    assert "profile_bottomk.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


def _arrays(n=3, S=4):
    return np.arange(n * S, dtype=np.uint64), np.ones(n * S)


def _smash(L, metric, weights=True, S=4, ex=False):
    m, w = _arrays(3, min(S, 8))
    out = np.zeros(9)
    args = (0, m.ctypes.data, w.ctypes.data if weights else None, 3, S, metric, out.ctypes.data)
    rc = L.hulk_smash_ex(*args, None) if ex else L.hulk_smash(*args)
    return rc, L.hulk_last_error(None).decode()


def _search(L, _lib, metric, weights=True, S=4):
    m, w = _arrays(3, min(S, 8))
    o = _lib.SearchOpts(k=2, metric=metric, role=0, flags=_lib.HULK_SEARCH_SELF, max_distance=-1.0)
    idx = np.zeros(6, dtype=np.uint32); d = np.zeros(6); c = np.zeros(3, dtype=np.uint32)
    rc = L.hulk_search(0, m.ctypes.data, w.ctypes.data if weights else None, 3, None, None, 0, S, ctypes.byref(o), idx.ctypes.data, d.ctypes.data,
                       c.ctypes.data, None)
    return rc, L.hulk_last_error(None).decode()


def _cluster(L, _lib, metric, weights=True, S=4):
    m, w = _arrays(3, min(S, 8))
    o = _lib.ClusterOpts(metric=metric, max_distance=0.5)
    lab = np.zeros(3, dtype=np.uint32)
    rc = L.hulk_cluster(0, m.ctypes.data, w.ctypes.data if weights else None, 3, S, ctypes.byref(o), lab.ctypes.data, None)
    return rc, L.hulk_last_error(None).decode()


def _dendrogram(L, _lib, metric, weights=True, S=4):
    m, w = _arrays(3, min(S, 8))
    o = _lib.DendrogramOpts(metric=metric)
    a = np.zeros(3, dtype=np.uint32); b = np.zeros(3, dtype=np.uint32); d = np.zeros(3); ne = ctypes.c_uint32(0)
    rc = L.hulk_dendrogram(0, m.ctypes.data, w.ctypes.data if weights else None, 3, S, ctypes.byref(o), a.ctypes.data, b.ctypes.data, d.ctypes.data,
                           ctypes.byref(ne), None)
    return rc, L.hulk_last_error(None).decode()


def _entry_points(L, _lib):
    return {"hulk_smash": lambda **kw: _smash(L, **kw), "hulk_smash_ex": lambda **kw: _smash(L, ex=True, **kw),
            "hulk_search": lambda **kw: _search(L, _lib, **kw), "hulk_cluster": lambda **kw: _cluster(L, _lib, **kw),
            "hulk_dendrogram": lambda **kw: _dendrogram(L, _lib, **kw)}


def test_metric_3_passes_the_argument_checks_of_the_five_array_entry_points():
    """HULK_ERR_NO_DEVICE (here) or 0 (where there is a device), never HULK_ERR_ARG; with weights or with NULL for them"""
    from hulk_amd import _lib
    L = _lib.load()
    for name, call in _entry_points(L, _lib).items():
        for weights in (True, False):
            rc, msg = call(metric=BOTTOMK, weights=weights)
            assert rc in (0, ERR_NO_DEVICE), (name, weights, rc, msg)
        # the other metrics need their weights as before, 2 and every other value stay no metric, and the sorted form has a size limit
        for metric in (0, 1):
            rc, msg = call(metric=metric, weights=False)
            assert rc == ERR_ARG and "NULL" in msg, (name, metric, rc, msg)
        for metric in (2, 4, -1):
            rc, msg = call(metric=metric)
            assert rc == ERR_ARG and msg.endswith("metric"), (name, metric, rc, msg)
        rc, msg = call(metric=BOTTOMK, S=_lib.HULK_MINHASH_MAX_SKETCH + 1)
        assert rc == ERR_ARG and "bottomk takes a sketch_size of at most 4096" in msg, (name, rc, msg)
    # the panel scores histosketch snapshots: it keeps refusing the metric
    assert L.hulk_panel_distances(0, None, None, 1, None, None, 1, 4, BOTTOMK, 0, None) == ERR_ARG


def test_python_binding_takes_the_metric_and_the_panel_refuses_it():
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    m = bi.random_set(3, 8, 1)
    for weights in (np.zeros((3, 8)), None):
        for call in (lambda: smash.distance_matrix(m, weights, "bottomk"), lambda: smash.search(m, weights, None, None, 2, "bottomk", self_search=True),
                     lambda: smash.cluster(m, weights, 0.5, "bottomk"), lambda: smash.dendrogram(m, weights, "bottomk")):
            try:
                call()
            except HulkError as e:
                assert e.code == ERR_NO_DEVICE, (e.code, e.message)
    with pytest.raises(HulkError, match="supplied distance metric is not available: bottomk") as ei:
        smash.panel_distances(m, np.zeros((3, 8)), m, np.zeros((3, 8)), "bottomk")
    assert ei.value.code == ERR_ARG and "['jaccard', 'weightedjaccard']" in ei.value.message
    with pytest.raises(HulkError, match=r"please select one of the following: \['jaccard', 'weightedjaccard', 'bottomk'\]"):
        smash.cluster(m, None, 0.5, "cosine")
    with pytest.raises((TypeError, ValueError)):
        smash.cluster(m, None, 0.5, "jaccard")                      # the other metrics read their weights


def _write(path, mins, k=21):
    """one file with a histosketch, a kmv and a khf signature of the same values (the writer computes the MD5 of each)"""
    from hulk_amd.sketchio import HULKdata, HistoSketch, KHFSketch, KMVSketch
    mins = np.asarray(mins, dtype=np.uint64)
    d = HULKdata()
    d.filename, d.banner_label = "reads.fq,", "blank"
    d.add(HistoSketch(k, mins % np.uint64(k ** 4), -np.ones(len(mins)), k ** 4, False))
    d.add(KMVSketch(k, len(mins), np.sort(mins)))
    d.add(KHFSketch(k, len(mins), mins))
    d.write_json(path)


def _sketch_dir(tmp_path, n=3, S=16):
    db = tmp_path / "db"
    db.mkdir()
    m = bi.random_set(n, S, 11)
    files = []
    for i in range(n):
        files.append(str(db / f"s{i}.json"))
        _write(files[-1], m[i])
    return db, files


NEW_TEXT = "bottomk is only supported for kmv sketches"


def test_files_forms_take_bottomk_with_kmv_and_refuse_it_for_the_others(tmp_path):
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    _, files = _sketch_dir(tmp_path)
    out = str(tmp_path / "o")
    forms = {"smash": lambda algo, metric: smash.smash(str(tmp_path / "db"), out, algo=algo, metric=metric),
             "search": lambda algo, metric: smash.search_files(files[:1], files, 2, algo=algo, metric=metric),
             "cluster": lambda algo, metric: smash.cluster_files(files, 0.5, algo=algo, metric=metric),
             "dendrogram": lambda algo, metric: smash.dendrogram_files(files, algo=algo, metric=metric)}
    for name, call in forms.items():
        try:
            call("kmv", "bottomk")
        except HulkError as e:
            assert e.code == ERR_NO_DEVICE, (name, e.code, e.message)
        for algo in ("histosketch", "khf"):
            with pytest.raises(HulkError) as ei:
                call(algo, "bottomk")
            assert ei.value.code == ERR_ARG and ei.value.message == NEW_TEXT, (name, algo, ei.value.message)
        # the precedence of "weighted jaccard is only supported for histosketches": behind the loader's own errors
        with pytest.raises(HulkError, match=r"specified k-mer size \(15\) not found"):
            smash.cluster_files(files, 0.5, ksize=15, algo="khf", metric="bottomk")
        with pytest.raises(HulkError, match="weighted jaccard is only supported for histosketches"):
            call("kmv", "weightedjaccard")
    # the library's own list of metrics (the Python layer checks first: ask the library directly)
    from hulk_amd import _lib
    L = _lib.load()
    err = ctypes.create_string_buffer(4096)
    arr = (ctypes.c_char_p * len(files))(*[os.fsencode(f) for f in files])
    rc = L.hulk_cluster_files(0, arr, len(files), 21, b"kmv", b"cosine", 0.5, 0, None, None, None, err, len(err))
    assert rc == ERR_ARG and err.value.decode() == "supplied distance metric is not available: cosine\nplease select one of the following: [jaccard weightedjaccard bottomk]"


def test_cli_takes_bottomk_with_kmv_and_refuses_it_for_the_others(tmp_path):
    from hulk_amd.__main__ import main
    db, files = _sketch_dir(tmp_path)
    out = str(tmp_path / "out")
    commands = {"smash": ["smash", "-d", str(db), "-o", out], "search": ["search", "-q", files[0], "-d", str(db), "-o", out],
                "cluster": ["cluster", "-d", str(db), "-o", out, "--maxDistance", "0.5"],
                "dendrogram": ["dendrogram", "-d", str(db), "-o", out, "--cut", "0.5"]}
    for name, argv in commands.items():
        for algo in ("histosketch", "khf"):
            buf = io.StringIO()
            with redirect_stdout(buf):
                rc = main(argv + ["-a", algo, "-m", "bottomk"])
            assert rc == 1 and "ERROR---> " + NEW_TEXT in buf.getvalue(), (name, algo, buf.getvalue())
        buf = io.StringIO()
        with redirect_stdout(buf):
            rc = main(argv + ["-a", "kmv", "-m", "bottomk"])
        assert NEW_TEXT not in buf.getvalue() and "not available" not in buf.getvalue(), (name, buf.getvalue())
        assert rc == 0 or "ERROR---> " in buf.getvalue(), (name, rc, buf.getvalue())      # (without a device: the library's "no device" error)
        buf = io.StringIO()
        with redirect_stdout(buf):
            rc = main(argv + ["-a", "kmv", "-m", "cosine"])
        assert rc == 1 and "please select one of the following: ['jaccard', 'weightedjaccard', 'bottomk']" in buf.getvalue(), (name, buf.getvalue())


def test_the_yardstick_is_the_counter_intersection_on_random_multisets():
    rng = np.random.default_rng(5)
    for rep in range(300):
        s = int(rng.integers(1, 70))
        spread = (1, 2, 5, 40)[rep % 4]
        a = rng.integers(0, spread * s, size=s).astype(np.uint64) + np.uint64((1 << 63) if rep % 2 else 0)
        b = rng.integers(0, spread * s, size=s).astype(np.uint64) + np.uint64((1 << 63) if rep % 2 else 0)
        assert bi.go_similarity(a, b) == bi.counter_similarity(a, b) == bi.go_similarity(b, a)
        assert bi.go_similarity(a, rng.permutation(a)) == 1.0
    # values are uint64, not float64
    assert bi.go_similarity([1 << 60], [(1 << 60) + 1]) == 0.0 and float(1 << 60) == float((1 << 60) + 1)
    # the hand-worked example of the issue: three against two counts two
    assert bi.go_similarity([9, 9, 9, 1, 2], [9, 9, 3, 4, 5]) == 2 / 5


def test_the_ragged_sizes_and_the_density_set_are_what_they_claim():
    """S = 257 .. 4095: more than one position per thread of the preparation and a ragged end; the set of tests/test_gpu_bottomk.py's
    density test holds a list of one value, a list of S values and a ladder between them"""
    bi.check_ragged_sizes()
    assert [bi.prep_split(s)[0] for s in bi.RAGGED_SIZES] == [2, 3, 4, 9, 16]
    bi.check_density_set(40, 1000)
    # the collection that goes through every user of the tile at S = 2049: ties abound, and its closest pair is one distance to follow
    m, D = bi.tied_collection(2049)
    a, b = bi.closest_pair(D)
    assert a < b and D[a, b] == D[~np.eye(len(D), dtype=bool)].min() and 0 < D[a, b] < 1
    assert not (D[a, :b] == D[a, b]).any(), "b is the first sketch at that distance from a"


@pytest.mark.parametrize("s", [1, 2, 31, 33, 50, 512, 4096] + list(bi.RAGGED_SIZES))
def test_the_planted_pairs_are_what_they_claim(s):
    from oracle import pyorc
    c = bi.tile_constants()
    assert c == dict(BK_W=32, PREP_THREADS=256, TS=32, TQ=64), "the tile's constants moved: look at what the planted runs straddle"
    names = set()
    for name, a, b, want in bi.planted_pairs(s):
        names.add(name)
        assert len(a) == len(b) == s
        assert bi.go_similarity(a, b) == want / s == bi.counter_similarity(a, b), (s, name)
        if name == "shifted by one rank":
            # what the position-wise jaccard of the two sorted lists says: nothing in common
            m = np.vstack([np.sort(a), np.sort(b)])
            assert pyorc.smash_matrix(m, np.zeros(m.shape), "jaccard")[0, 1] == 1.0 and bi.distance(a, b) == 1.0 - (s - 1) / s
        if name.startswith("runs across every window") and s > c["BK_W"]:
            sa = np.sort(a)
            assert all(sa[p - 1] == sa[p] for p in range(c["BK_W"], s - 1, c["BK_W"])), "no run across a window boundary"
        if name.startswith("runs across the preparation") and s >= 4:
            e = -(-s // c["PREP_THREADS"])
            sa = np.sort(a)
            assert sum(sa[p - 1] == sa[p] for p in range(e, s, e)) >= (s // e) // 3, "too few runs across the preparation's boundaries"
    assert {"identical", "disjoint", "shifted by one rank", "all equal", "2^60 against 2^60 + 1", "MaxUint64 and 0"} <= names
    if s <= 512:
        m = bi.planted_set(97, s)
        D = bi.matrix(m)
        assert D.shape == (97, 97) and (np.diag(D) == 0).all() and np.array_equal(D, D.T)


def test_the_kernels_arithmetic_on_the_host_under_sanitizers(tmp_path):
    """hulk_bottomk_merge.h is HIP-free: the same text in a stand-alone program — the sorting network at every length, the run-length
    merge against kmv.go's loop, the tile's windows against the merge of whole lists"""
    exe = str(tmp_path / "bottomk_host")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan",      # (the runtimes inside the program: it is whole on its own)
                        "-I", os.path.join(ROOT, "hulk_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "bottomk_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stdout.count(": ok") == 6, r.stdout + r.stderr[-3000:]
