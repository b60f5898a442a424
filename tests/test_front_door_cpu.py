"""The front door of the sketch-collection file commands: which message wins when a call breaks two rules at once.

Every *_files entry point of the library checks its names (metric, algorithm, linkage method), then its own arguments, then loads
the files, then the metric against the loaded algorithm.  These cases call the raw ctypes entry points, bypassing Python's own
checks, and fail before any device call: no GPU needed.  The Python *_files functions and the CLI subcommands that check the
names themselves are held to their own (list-repr) texts.
"""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

ERR_ARG = -30
METRIC_MSG = "supplied distance metric is not available: cosine\nplease select one of the following: [jaccard weightedjaccard bottomk]"
ALGO_MSG = "supplied algorithm not available: foo\nplease select one of the following: [histosketch kmv khf]"
LINKAGE_MSG = "supplied linkage is not available: ward\nplease select one of the following: [single complete average]"
WJ_MSG = "weighted jaccard is only supported for histosketches"
BK_MSG = "bottomk is only supported for kmv sketches"
PY_METRIC_MSG = "supplied distance metric is not available: cosine\nplease select one of the following: ['jaccard', 'weightedjaccard', 'bottomk']"
PY_ALGO_MSG = "supplied algorithm not available: foo\nplease select one of the following: ['histosketch', 'kmv', 'khf']"
PY_LINKAGE_MSG = "supplied linkage is not available: ward\nplease select one of the following: ['single', 'complete', 'average']"
NAN = float("nan")


def _write(path, mins, k=21):
    """one file with a histosketch, a kmv and a khf signature of the same values"""
    from hulk_amd.sketchio import HULKdata, HistoSketch, KHFSketch, KMVSketch
    mins = np.asarray(mins, dtype=np.uint64)
    d = HULKdata()
    d.filename, d.banner_label = "reads.fq,", "blank"
    d.add(HistoSketch(k, mins % np.uint64(k ** 4), -np.ones(len(mins)), k ** 4, False))
    d.add(KMVSketch(k, len(mins), np.sort(mins)))
    d.add(KHFSketch(k, len(mins), mins))
    d.write_json(path)


@pytest.fixture(scope="module")
def sk(tmp_path_factory):
    """three sketch files of S = 8, one of S = 16, one that does not load and a path that does not exist"""
    d = tmp_path_factory.mktemp("front_door")
    rng = np.random.default_rng(5)
    files = []
    for i in range(3):
        files.append(str(d / f"s{i}.json"))
        _write(files[-1], rng.integers(1, 2 ** 40, 8))
    long_file = str(d / "long.json")
    _write(long_file, rng.integers(1, 2 ** 40, 16))
    bad = str(d / "bad.json")
    with open(bad, "w") as fh:
        fh.write("{not json")
    return dict(dir=str(d), files=files, long=long_file, bad=bad, missing=str(d / "missing.json"), out=str(d / "out"))


def _lib():
    from hulk_amd import _lib as lib
    return lib, lib.load()


def _arr(paths):
    return (ctypes.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])


def _err():
    return ctypes.create_string_buffer(4096)


def smash_files(paths, algo, metric):
    _, L = _lib()
    e = _err()
    rc = L.hulk_smash_files(0, _arr(paths), len(paths), 21, algo.encode(), metric.encode(), 0, None, None, None, None, e, len(e))
    return rc, e.value.decode()


def search_files(q, db, algo, metric, k=2, role=0, flags=0):
    _, L = _lib()
    e = _err()
    da, nd = (None, 0) if db is None else (_arr(db), len(db))
    rc = L.hulk_search_files(0, _arr(q), len(q), da, nd, 21, algo.encode(), metric.encode(), role, k, -1.0, flags, 0, None,
                             None, None, None, None, e, len(e))
    return rc, e.value.decode()


def index_build_files(paths, algo, opts=True):
    lib, L = _lib()
    e = _err()
    o = lib.IndexOpts(max_distance=0.5, bands=0, metric=lib.HULK_METRIC_JACCARD)
    h = ctypes.c_void_p()
    rc = L.hulk_index_build_files(0, _arr(paths), len(paths), 21, algo.encode(), 0, ctypes.byref(o) if opts else None, ctypes.byref(h), e, len(e))
    assert not h.value
    return rc, e.value.decode()


def cluster_files(paths, algo, metric, max_distance=0.5):
    _, L = _lib()
    e = _err()
    rc = L.hulk_cluster_files(0, _arr(paths), len(paths), 21, algo.encode(), metric.encode(), max_distance, 0, None, None, None, e, len(e))
    return rc, e.value.decode()


def links_files(paths, algo, metric, max_distance=0.5, flags=0):
    _, L = _lib()
    e = _err()
    h = ctypes.c_void_p()
    rc = L.hulk_links_files(0, _arr(paths), len(paths), 21, algo.encode(), metric.encode(), max_distance, flags, 0, 0, None, ctypes.byref(h),
                            None, e, len(e))
    assert not h.value
    return rc, e.value.decode()


def dendrogram_files(paths, algo, metric, cut=NAN, cut_path=None):
    _, L = _lib()
    e = _err()
    rc = L.hulk_dendrogram_files(0, _arr(paths), len(paths), 21, algo.encode(), metric.encode(), 0, None, cut,
                                 None if cut_path is None else os.fsencode(cut_path), None, None, None, None, None, e, len(e))
    return rc, e.value.decode()


def linkage_files(paths, algo, metric, method="single", cut=NAN, cut_path=None):
    _, L = _lib()
    e = _err()
    rc = L.hulk_linkage_files(0, _arr(paths), len(paths), 21, algo.encode(), metric.encode(), method.encode(), 0, None, cut,
                              None if cut_path is None else os.fsencode(cut_path), None, None, None, None, None, None, e, len(e))
    return rc, e.value.decode()


def _metric_entries(sk):
    """the entry points that take a metric: name -> fn(paths, algo, metric)"""
    return {"smash": smash_files, "search": lambda p, a, m: search_files(p[:1], p, a, m), "cluster": cluster_files,
            "links": links_files, "dendrogram": dendrogram_files, "linkage": linkage_files}


def _own_bad_args(sk):
    """per entry point, calls that break one of the entry's own argument rules: name -> [(fn(paths, algo), message)]"""
    self_ = 1
    return {
        "search": [(lambda p, a: search_files(p, p, a, "jaccard", k=0), "hulk_search: k must be 1 .. 64"),
                   (lambda p, a: search_files(p, p, a, "jaccard", role=7), "hulk_search: role"),
                   (lambda p, a: search_files(p, p, a, "jaccard", flags=2), "hulk_search: unknown flags"),
                   (lambda p, a: search_files(p, p, a, "jaccard", flags=self_), "hulk_search: HULK_SEARCH_SELF takes no database")],
        "cluster": [(lambda p, a: cluster_files(p, a, "jaccard", max_distance=2.0), "hulk_cluster: max_distance must be in [0, 1]")],
        "links": [(lambda p, a: links_files(p, a, "jaccard", max_distance=2.0), "hulk_links: max_distance must be in [0, 1]"),
                  (lambda p, a: links_files(p, a, "jaccard", flags=0x80), "hulk_links: unknown flags")],
        "dendrogram": [(lambda p, a: dendrogram_files(p, a, "jaccard", cut=2.0, cut_path=sk["out"]),
                        "hulk_dendrogram: cut_distance must be in [0, 1] (or NaN: no cut)"),
                       (lambda p, a: dendrogram_files(p, a, "jaccard", cut=0.5), "hulk_dendrogram: a cut_distance without a cut_csv_path")],
        "linkage": [(lambda p, a: linkage_files(p, a, "jaccard", cut=2.0, cut_path=sk["out"]),
                     "hulk_linkage: cut_distance must be in [0, 1] (or NaN: no cut)"),
                    (lambda p, a: linkage_files(p, a, "jaccard", cut=0.5), "hulk_linkage: a cut_distance without a cut_csv_path"),
                    (lambda p, a: linkage_files(p, a, "jaccard", method="ward"), LINKAGE_MSG)],
    }


def test_a_bad_metric_wins_over_a_bad_algorithm(sk):
    for name, fn in _metric_entries(sk).items():
        assert fn(sk["files"], "foo", "cosine") == (ERR_ARG, METRIC_MSG), name


def test_a_bad_algorithm_wins_over_the_entrys_own_bad_argument(sk):
    for name, cases in _own_bad_args(sk).items():
        for fn, _ in cases:
            assert fn(sk["files"], "foo") == (ERR_ARG, ALGO_MSG), name
    # the entry points without a metric check the algorithm first too
    assert index_build_files(sk["files"], "foo") == (ERR_ARG, ALGO_MSG)


def test_linkage_a_bad_method_wins_over_a_bad_cut(sk):
    assert linkage_files(sk["files"], "kmv", "jaccard", method="ward", cut=2.0, cut_path=sk["out"]) == (ERR_ARG, LINKAGE_MSG)
    assert linkage_files(sk["files"], "kmv", "jaccard", method="ward", cut=0.5) == (ERR_ARG, LINKAGE_MSG)


def test_the_entrys_own_arguments_are_checked_before_loading(sk):
    paths = sk["files"] + [sk["missing"]]
    for name, cases in _own_bad_args(sk).items():
        for fn, msg in cases:
            assert fn(paths, "kmv") == (ERR_ARG, msg), name
    # and the missing file itself is the loader's error
    for name, fn in _metric_entries(sk).items():
        rc, msg = fn(paths, "kmv", "jaccard")
        assert rc == ERR_ARG and msg.startswith("open " + sk["missing"] + ": "), (name, msg)


def test_a_load_error_wins_over_the_metric_rules_which_follow_it(sk):
    for name, fn in _metric_entries(sk).items():
        rc, msg = fn(sk["files"] + [sk["bad"]], "kmv", "weightedjaccard")
        assert rc == ERR_ARG and msg.startswith("malformed sketch file (") and msg.endswith(sk["bad"] + "\n"), (name, msg)
        assert fn(sk["files"], "kmv", "weightedjaccard") == (ERR_ARG, WJ_MSG), name
        assert fn(sk["files"], "khf", "bottomk") == (ERR_ARG, BK_MSG), name
        assert fn(sk["files"], "histosketch", "bottomk") == (ERR_ARG, BK_MSG), name


def test_search_length_mismatch_and_the_single_query(sk):
    files = sk["files"]
    assert search_files([sk["long"]], files, "kmv", "weightedjaccard") == (ERR_ARG, "sketch length mismatch: 16 vs 8\n")
    # a single query file loads; smash still wants two
    assert search_files(files[:1], None, "kmv", "weightedjaccard", flags=1) == (ERR_ARG, WJ_MSG)
    assert smash_files(files[:1], "kmv", "weightedjaccard") == (ERR_ARG, "1 sketches found in the supplied directory, HULK needs at least 2 to smash!\n")


def test_index_build_files_null_opts_before_the_algorithm(sk):
    assert index_build_files(sk["files"], "foo", opts=False) == (ERR_ARG, "NULL")


def test_python_files_forms_keep_their_own_texts(sk):
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    f = sk["files"]
    forms = {"smash": lambda a, m: smash.smash(sk["dir"], sk["out"], algo=a, metric=m),
             "search_files": lambda a, m: smash.search_files(f[:1], f, 2, algo=a, metric=m),
             "cluster_files": lambda a, m: smash.cluster_files(f, 0.5, algo=a, metric=m),
             "links_files": lambda a, m: smash.links_files(f, 0.5, algo=a, metric=m),
             "dendrogram_files": lambda a, m: smash.dendrogram_files(f, algo=a, metric=m),
             "linkage_files": lambda a, m: smash.linkage_files(f, "single", algo=a, metric=m)}
    for name, call in forms.items():
        for (a, m), msg in (((("foo", "cosine")), PY_METRIC_MSG), (("foo", "jaccard"), PY_ALGO_MSG)):
            with pytest.raises(HulkError) as ei:
                call(a, m)
            assert (ei.value.code, ei.value.message) == (ERR_ARG, msg), name
    with pytest.raises(HulkError) as ei:
        smash.linkage_files(f, "ward", algo="kmv")
    assert ei.value.message == PY_LINKAGE_MSG
    # the forms that leave the names to the library carry the library's texts
    with pytest.raises(HulkError) as ei:
        smash.Index.build_files(f, 0.5, algo="foo")
    assert (ei.value.code, ei.value.message) == (ERR_ARG, ALGO_MSG)
    with pytest.raises(HulkError) as ei:
        smash.load_sketches(f, algo="foo")
    assert ei.value.message.startswith("specified algorithm (foo) not found in the supplied sketch: ")


def test_stats_dicts_carry_every_field_under_its_name():
    from hulk_amd import _lib as lib
    from hulk_amd.smash import _stats
    keys = {lib.SearchStats: ["seconds_total", "kernel_ms_dist", "kernel_ms_select", "strips", "query_blocks"],
            lib.IndexSearchStats: ["seconds_total", "kernel_ms_keys", "kernel_ms_probe", "kernel_ms_verify", "kernel_ms_select", "candidates",
                                   "within", "query_blocks", "pieces"],
            lib.ClusterStats: ["seconds_total", "kernel_ms_link", "kernel_ms_flatten", "links", "bands", "clusters"],
            lib.LinksStats: ["seconds_total", "kernel_ms_count", "kernel_ms_fill", "edges", "bands", "max_degree"],
            lib.DendrogramStats: ["seconds_total", "kernel_ms_offer", "kernel_ms_fold", "rounds", "bands", "edges", "components"],
            lib.LinkageStats: ["seconds_total", "kernel_ms_matrix", "kernel_ms_merge", "merges", "components", "rows_rescanned"]}
    for struct, names in keys.items():
        st = struct()
        for i, (name, _) in enumerate(struct._fields_):
            setattr(st, name, i + 1)
        assert _stats(st) == {name: i + 1 for i, name in enumerate(names)}, struct.__name__


def test_cli_subcommands_keep_their_texts(sk):
    from hulk_amd.__main__ import main
    d, out = sk["dir"], sk["out"]
    commands = {"smash": ["smash", "-d", d, "-o", out], "search": ["search", "-q", sk["files"][0], "-d", d, "-o", out],
                "cluster": ["cluster", "-d", d, "-o", out, "--maxDistance", "0.5"],
                "links": ["links", "-d", d, "-o", out, "--maxDistance", "0.5"],
                "dendrogram": ["dendrogram", "-d", d, "-o", out], "linkage": ["dendrogram", "-d", d, "-o", out, "--linkage", "average"]}
    for name, argv in commands.items():
        for extra, msg in ((["-a", "foo", "-m", "cosine"], PY_METRIC_MSG), (["-a", "foo"], PY_ALGO_MSG)):
            buf = io.StringIO()
            with redirect_stdout(buf):
                rc = main(argv + extra)
            assert rc == 1 and "ERROR---> " + msg + "\n" in buf.getvalue(), (name, buf.getvalue())
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = main(["dendrogram", "-d", d, "-o", out, "--linkage", "ward"])
    assert rc == 1 and "ERROR---> " + PY_LINKAGE_MSG + "\n" in buf.getvalue(), buf.getvalue()
    for mode in ("create", "search"):
        buf = io.StringIO()
        with redirect_stdout(buf):
            rc = main(["index", "-r", mode, "-n", out, "-d", d, "-j", "0.9", "-a", "foo"])
        assert rc == 1 and "ERROR---> " + PY_ALGO_MSG + "\n" in buf.getvalue(), (mode, buf.getvalue())
