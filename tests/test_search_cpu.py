"""Nearest-neighbour search (hulk_search, hulk_search_files), the parts that need no GPU: the header declares the entry points and the
built library exports them, every argument error is refused with its text before the library looks for a device, the directory form
loads a one-file query set and reports the reference's texts, the CLI refuses a bad --top and an unknown metric, the C++ host
mirror's driver compiles and links."""
import ctypes
import io
import os
import re
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

import search_inputs as si
from conftest import ROOT

ENTRY_POINTS = ("hulk_search", "hulk_search_files")
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
    assert re.search(r"#define HULK_SEARCH_MAX_K 64u\b", code) and re.search(r"#define HULK_SEARCH_SELF 1u\b", code)
    assert (_lib.HULK_SEARCH_MAX_K, _lib.HULK_SEARCH_SELF) == (64, 1)
    assert "typedef struct hulk_search_opts" in code and "typedef struct hulk_search_stats" in code
    assert "#define HULK_ABI_VERSION 4" in hdr, "additions only: the ABI version stays"
    L.hulk_abi_version.restype = ctypes.c_int
    assert L.hulk_abi_version() == 4
    # the structs as the header lays them out
    assert ctypes.sizeof(_lib.SearchOpts) == 64 and _lib.SearchOpts.max_distance.offset == 16 and _lib.SearchOpts.reserved.offset == 32
    assert ctypes.sizeof(_lib.SearchStats) == 32 and _lib.SearchStats.strips.offset == 24
    if os.path.exists(_lib.EXP_LIB_PATH):
        X = ctypes.CDLL(_lib.EXP_LIB_PATH)
        assert all(hasattr(X, n) for n in ENTRY_POINTS)


def _call(L, _lib, *, k=3, metric=0, role=0, flags=0, reserved=(0, 0, 0, 0), scratch=0, m=2, n_db=3, S=4, q=True, db=True, out=True, opts=True):
    qm = np.arange(m * S + 1, dtype=np.uint64); qw = np.ones(m * S + 1)
    dm = np.arange(n_db * S + 1, dtype=np.uint64); dw = np.ones(n_db * S + 1)
    idx = np.zeros(max(m, 1) * 64, dtype=np.uint32); dist = np.zeros(max(m, 1) * 64); cnt = np.zeros(max(m, 1), dtype=np.uint32)
    o = _lib.SearchOpts(k=k, metric=metric, role=role, flags=flags, max_distance=-1.0, scratch_bytes=scratch)
    for i, v in enumerate(reserved):
        o.reserved[i] = v
    rc = L.hulk_search(0, qm.ctypes.data if q else None, qw.ctypes.data if q else None, m, dm.ctypes.data if db else None,
                       dw.ctypes.data if db else None, n_db, S, ctypes.byref(o) if opts else None, idx.ctypes.data if out else None,
                       dist.ctypes.data if out else None, cnt.ctypes.data, None)
    return rc, L.hulk_last_error(None).decode()


def test_every_argument_error_is_refused_with_its_text_before_a_device_is_looked_for():
    """each of these returns HULK_ERR_ARG, not HULK_ERR_NO_DEVICE: here there is no device, and the argument checks come first"""
    from hulk_amd import _lib
    L = _lib.load()
    cases = [
        (dict(q=False), "hulk_search: NULL"),
        (dict(out=False), "hulk_search: NULL"),
        (dict(opts=False), "hulk_search: NULL"),
        (dict(k=0), "k must be 1 .. 64"),
        (dict(k=65), "k must be 1 .. 64"),
        (dict(m=0), "m, n_db and sketch_size must be positive"),
        (dict(n_db=0), "m, n_db and sketch_size must be positive"),
        (dict(S=0), "m, n_db and sketch_size must be positive"),
        (dict(metric=2), "hulk_search: metric"),
        (dict(metric=-1), "hulk_search: metric"),
        (dict(role=2), "hulk_search: role"),
        (dict(flags=2), "unknown flags"),
        (dict(reserved=(0, 0, 0, 1)), "reserved fields must be zero"),
        (dict(reserved=(7, 0, 0, 0)), "reserved fields must be zero"),
        (dict(flags=_lib.HULK_SEARCH_SELF), "HULK_SEARCH_SELF takes no database"),
        (dict(db=False), "no database (and no HULK_SEARCH_SELF)"),
        (dict(scratch=1), "too small for one tile"),
        (dict(scratch=64 * (4 * 32 + 32 * 8) - 1), "too small for one tile"),        # one byte short of 32 queries x 64 sketches at S = 4
    ]
    for kw, text in cases:
        rc, msg = _call(L, _lib, **kw)
        assert rc == ERR_ARG and text in msg, (kw, rc, msg)
    # the smallest scratch that holds a tile gets past the argument checks (and then finds no device here, or runs)
    rc, msg = _call(L, _lib, scratch=64 * (4 * 32 + 32 * 8))
    assert rc in (0, ERR_NO_DEVICE), (rc, msg)
    rc, msg = _call(L, _lib, flags=_lib.HULK_SEARCH_SELF, db=False)
    assert rc in (0, ERR_NO_DEVICE), (rc, msg)


def test_python_binding_refuses_without_a_device():
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    rng = np.random.default_rng(1)
    m = rng.integers(0, 100, size=(3, 8)).astype(np.uint64); w = -rng.random((3, 8))
    for k in (0, 65, -1):
        with pytest.raises(HulkError, match="k must be 1 .. 64"):
            smash.search(m, w, m, w, k)
    with pytest.raises(HulkError, match="supplied distance metric is not available: cosine"):
        smash.search(m, w, m, w, 3, metric="cosine")
    with pytest.raises(HulkError, match="sketch length mismatch: 8 vs 7"):
        smash.search(m, w, m[:, :7], w[:, :7], 3)
    with pytest.raises(ValueError):
        smash.search(m, w, m, w, 3, role="diagonal")
    with pytest.raises(ValueError):
        smash.search(m, w, m, w, 3, self_search=True)


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


def test_directory_form_loads_a_single_query_and_reports_the_reference_texts(tmp_path):
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    db = _sketch_files(tmp_path, 3, 16)
    q = _sketch_files(tmp_path, 1, 16, seed=4, prefix="q")
    # one query file, and a database of one file: "needs at least 2" is smash's rule, not the search's.  Loading is all that can
    # succeed without a device
    for database in (db, db[:1]):
        try:
            smash.search_files(q, database, 2)
        except HulkError as e:
            assert e.code == ERR_NO_DEVICE, (e.code, e.message)
    with pytest.raises(HulkError, match="HULK needs at least 2 to smash"):       # the loader of `smash` keeps its rule
        smash.load_sketches(q)
    with pytest.raises(HulkError) as ei:
        smash.search_files([], db, 2)
    assert ei.value.code == ERR_ARG and ei.value.message == "no sketch files supplied\n"
    # a bad MD5 in either set: LoadHULKdata's text
    bad = str(tmp_path / "bad.json")
    open(bad, "w").write(open(db[0]).read().replace('"mins": [', '"mins": [1, ', 1))
    for qs, ds in (([bad], db), (q, db + [bad])):
        with pytest.raises(HulkError) as ei:
            smash.search_files(qs, ds, 2)
        assert ei.value.code == ERR_ARG and re.fullmatch(r"md5sum mismatch: [0-9a-f]{32} vs\. [0-9a-f]{32}\n", ei.value.message), ei.value.message
    # different lengths across the sets: GetDistance's text, the queries' length first
    short = _sketch_files(tmp_path, 2, 12, seed=5, prefix="s")
    with pytest.raises(HulkError) as ei:
        smash.search_files(short, db, 2)
    assert ei.value.code == ERR_ARG and ei.value.message == "sketch length mismatch: 12 vs 16\n"
    with pytest.raises(HulkError) as ei:
        smash.search_files(q, short, 2)
    assert ei.value.message == "sketch length mismatch: 16 vs 12\n"
    # ... and inside one set the loader's own check
    with pytest.raises(HulkError) as ei:
        smash.search_files(q, db + short[:1], 2)
    assert ei.value.message == "sketch length mismatch: 16 vs 12\n"
    # the rest of the directory form's argument checks
    with pytest.raises(HulkError, match="k must be 1 .. 64"):
        smash.search_files(q, db, 65)
    with pytest.raises(HulkError, match="supplied algorithm not available: minhash"):
        smash.search_files(q, db, 2, algo="minhash")
    with pytest.raises(HulkError, match=r"specified k-mer size \(15\) not found"):
        smash.search_files(q, db, 2, ksize=15)


def test_cli_refuses_a_bad_top_and_an_unknown_metric(tmp_path):
    from hulk_amd.__main__ import main
    db = tmp_path / "db"
    db.mkdir()
    _sketch_files(db, 2, 8)
    out = str(tmp_path / "out")
    for extra, text in ((["--top", "0"], "--top must be between 1 and 64"), (["--top", "65"], "--top must be between 1 and 64"),
                        (["-m", "cosine"], "supplied distance metric is not available: cosine")):
        buf = io.StringIO()
        with redirect_stdout(buf):
            rc = main(["search", "-q", str(db), "-d", str(db), "-o", out] + extra)
        assert rc == 1
        assert "ERROR---> " + text in buf.getvalue(), buf.getvalue()
        assert sorted(os.listdir(tmp_path)) == ["db"], "nothing is written"


# ---- the inputs that take the selection beyond one pass are a test (tests/search_inputs.py, on the yardstick alone) -------------------
@pytest.mark.parametrize("s,metric", si.LONG_CASES)
def test_the_long_strips_are_what_they_claim(s, metric):
    si.check_long_strips(s, metric)
    # the scratch that makes two strips of 576 + 524 sketches, by search_plan's own rule (Mb = 32 for five queries)
    per_sketch = 32 * s + 8 * 32
    assert si.strip_scratch(s) // per_sketch // 64 * 64 == si.STRIP == 576 and -(-si.LONG_P // si.STRIP) == 2
    text = open(os.path.join(ROOT, "hulk_amd", "csrc", "hulk_search.hip")).read()
    assert "Pb = budget / ((uint64_t)S * 32 + Mb * 8) / 64 * 64;" in text, "search_plan moved: look at strip_scratch"


@pytest.mark.parametrize("s,metric", si.LONG_CASES)
def test_the_database_orders_and_the_self_search_limit_are_what_they_claim(s, metric):
    for role in si.ROLES:
        entered = si.check_orders(s, metric, role)
        print(f"S {s} {metric} {role}: candidates that enter query 0's list of {si.LONG_K}: {entered}")
        assert entered["ascending"] == entered["identical"] == si.LONG_K < entered["copies"] < entered["descending"]
        lim, cut, free = si.check_self_search(s, metric, role)
        print(f"S {s} {metric} {role}: max_distance {lim!r} leaves {cut[2].mean():.1f} hits a query")


def test_the_replay_of_the_selection_counts_insertions():
    assert si.insertions(np.array([0.5, 0.4, 0.3, 0.2]), 2) == 4            # descending: every candidate enters
    assert si.insertions(np.array([0.2, 0.3, 0.4, 0.5]), 2) == 2            # ascending: the first K
    assert si.insertions(np.array([0.3, 0.3, 0.3, 0.3]), 2) == 2            # ties: a later index never beats an earlier one
    assert si.insertions(np.array([0.3, np.nan, 0.1, 0.3, 0.2]), 2) == 3    # NaN is no candidate
    D = np.array([[0.3, np.nan, 0.1, 0.3, 0.2]])
    assert si.select(D, 2)[0].tolist() == [[2, 4]] and si.select(D, 4)[2].tolist() == [4]


def test_cpp_search_driver_compiles_and_links(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "search_driver.cpp"), "-o", str(tmp_path / "search_driver"),
           "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
