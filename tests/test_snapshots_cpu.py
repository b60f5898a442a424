"""Sketch snapshots, the parts that need no GPU: the header declares the entry points and the built library exports them, the C++
host mirror compiles and links, `--streamEvery` is parsed and refused without an interval, the snapshot writer's files go
through load_hulk_data unchanged."""
import ctypes
import io
import json
import os
import re
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT

ENTRY_POINTS = ("hulk_set_snapshots", "hulk_snapshot_count", "hulk_get_snapshots", "hulk_set_snapshot_callback", "hulk_poll_snapshots")


def test_header_declares_and_library_exports_the_entry_points():
    from hulk_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hulk_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(hulk_ctx \*ctx" % name, code), f"{name} is not declared in hulk_hip.h"
        assert hasattr(L, name), f"libhulkhip.so does not export {name}"
        assert name in _lib.ABI_SYMBOLS
    assert "typedef struct hulk_snapshot_info" in code and "(*hulk_snapshot_fn)" in code
    assert "#define HULK_ABI_VERSION 4" in hdr, "additions only: the ABI version stays"
    assert ctypes.sizeof(_lib.SnapshotInfo) == 16 and _lib.SnapshotInfo.n_reads.offset == 8
    if os.path.exists(_lib.EXP_LIB_PATH):
        X = ctypes.CDLL(_lib.EXP_LIB_PATH)
        assert all(hasattr(X, n) for n in ENTRY_POINTS)


def test_entry_points_refuse_a_null_context():
    """reachable without a GPU: every entry point checks its context first (HULK_ERR_ARG, no crash)"""
    from hulk_amd import _lib
    L = _lib.load()
    assert L.hulk_set_snapshots(None, 1, 0) == -30
    assert L.hulk_snapshot_count(None, None, None) == -30
    assert L.hulk_get_snapshots(None, 0, 0, None, None, None) == -30
    assert L.hulk_poll_snapshots(None, None) == -30
    assert L.hulk_set_snapshot_callback(None, _lib.SNAPSHOT_FN(lambda *a: 0), None) == -30


def test_cpp_snapshot_driver_compiles_and_links(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "snapshot_driver.cpp"), "-o", str(tmp_path / "snapshot_driver"),
           "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]


def test_stream_every_is_parsed_and_needs_an_interval(tmp_path):
    from hulk_amd.__main__ import main
    fq = tmp_path / "r.fq"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    for extra in ([], ["--stream", "--log", str(tmp_path / "log.txt")]):
        buf = io.StringIO()
        with redirect_stdout(buf):
            rc = main(["sketch", "-f", str(fq), "-o", str(tmp_path / "out"), "--streamEvery", "3"] + extra)
        assert rc == 1
        text = buf.getvalue() if not extra else open(tmp_path / "log.txt").read()
        assert text.rstrip().endswith("ERROR---> --streamEvery needs an interval (-i)")
        assert not os.path.exists(str(tmp_path / "out") + ".snapshots") and not os.path.exists(str(tmp_path / "out") + ".json")
    with pytest.raises(SystemExit):                                # argparse: N is an integer
        with redirect_stdout(io.StringIO()), open(os.devnull, "w") as null:
            import contextlib
            with contextlib.redirect_stderr(null):
                main(["sketch", "-f", str(fq), "--streamEvery", "often"])


def test_snapshot_writer_round_trip(tmp_path):
    from hulk_amd import HistoSketch
    from hulk_amd.sketchio import HULKdata, load_hulk_data, md5sum, snapshot_document, snapshot_path
    out = str(tmp_path / "run")
    assert snapshot_path(out, 7) == out + ".snapshots/00000007.json"
    assert snapshot_path(out, 123456789) == out + ".snapshots/123456789.json"
    assert sorted(snapshot_path(out, o) for o in (10, 9, 100)) == [snapshot_path(out, o) for o in (9, 10, 100)]
    mins = np.array([5, 0, 194480, 2 ** 63 + 1], dtype=np.uint64)
    w = np.array([-0.25, 1.7976931348623157e308, 3e-9, -1.5e-7])
    os.makedirs(out + ".snapshots")
    d = snapshot_document(HistoSketch(21, mins, w, 194481, True), "a.fq,b<c>.fq,", "blank")
    d.write_json(snapshot_path(out, 7))
    back = load_hulk_data(snapshot_path(out, 7))
    (algo, hs), = back.signatures
    assert algo == "histosketch" and back.filename == "a.fq,b<c>.fq," and back.banner_label == "blank"
    assert np.array_equal(hs.mins, mins) and np.array_equal(hs.weights.view(np.uint64), w.view(np.uint64))
    assert hs.md5sum == md5sum(mins) and hs.concept_drift is True and hs.num_histogram_bins == 194481
    # the document of the end of the run is the same writer: same fields in the same order
    end = HULKdata(); end.add(HistoSketch(21, mins, w, 194481, True)); end.filename = "a.fq,b<c>.fq,"; end.banner_label = "blank"
    assert end.dumps() == d.dumps()
    # --stream prints it on one line: same JSON, every number spelled as in the file
    line = d.dumps_line()
    assert "\n" not in line and json.loads(line) == json.load(open(snapshot_path(out, 7)))
    assert "1.7976931348623157e+308" in line and "1.5e-7" in line and "\\u003c" in line
