"""Scoring sketch snapshots against a panel, the parts that need no GPU: the header declares the entry points and the role
constants and the built library exports them, every entry point refuses a NULL context, `--panel` is refused without
`--streamEvery`, the C++ host mirror compiles and links."""
import ctypes
import io
import os
import re
import subprocess
from contextlib import redirect_stdout

from conftest import ROOT

ENTRY_POINTS = ("hulk_set_panel", "hulk_get_snapshot_distances", "hulk_set_snapshot_panel_callback", "hulk_panel_distances")


def test_header_declares_and_library_exports_the_entry_points():
    from hulk_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hulk_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        first = r"int device" if name == "hulk_panel_distances" else r"hulk_ctx \*ctx"
        assert re.search(r"\bint %s\s*\(%s" % (name, first), code), f"{name} is not declared in hulk_hip.h"
        assert hasattr(L, name), f"libhulkhip.so does not export {name}"
        assert name in _lib.ABI_SYMBOLS
    assert "(*hulk_snapshot_panel_fn)" in code                     # the fifth new name of the header: the callback's type
    assert re.search(r"#define HULK_PANEL_ROW 0\b", code) and re.search(r"#define HULK_PANEL_COLUMN 1\b", code)
    assert (_lib.HULK_PANEL_ROW, _lib.HULK_PANEL_COLUMN) == (0, 1)
    m = re.search(r"#define HULK_PANEL_MAX (\d+)u?\b", code)
    assert m and int(m.group(1)) == _lib.HULK_PANEL_MAX
    assert "#define HULK_ABI_VERSION 4" in hdr, "additions only: the ABI version stays"
    if os.path.exists(_lib.EXP_LIB_PATH):
        X = ctypes.CDLL(_lib.EXP_LIB_PATH)
        assert all(hasattr(X, n) for n in ENTRY_POINTS)


def test_entry_points_refuse_a_null_context():
    """reachable without a GPU: every entry point that takes a context checks it first (HULK_ERR_ARG, no crash)"""
    from hulk_amd import _lib
    L = _lib.load()
    assert L.hulk_set_panel(None, None, None, 0, 0, 0, 0) == -30
    assert L.hulk_get_snapshot_distances(None, 0, 0, None) == -30
    assert L.hulk_set_snapshot_panel_callback(None, _lib.SNAPSHOT_PANEL_FN(lambda *a: 0), None) == -30
    # the context-free one checks its arguments before it looks for a device
    assert L.hulk_panel_distances(0, None, None, 1, None, None, 1, 4, 7, 0, None) == -30       # metric
    assert L.hulk_panel_distances(0, None, None, 1, None, None, 1, 4, 0, 2, None) == -30       # role
    assert L.hulk_panel_distances(0, None, None, 1, None, None, _lib.HULK_PANEL_MAX + 1, 4, 0, 0, None) == -30
    assert L.hulk_panel_distances(0, None, None, 1, None, None, 1, 4, 0, 0, None) == -30       # NULL arrays


def test_panel_needs_stream_every(tmp_path):
    from hulk_amd.__main__ import main
    fq = tmp_path / "r.fq"
    fq.write_text("@r\nACGT\n+\nIIII\n")
    panel = tmp_path / "panel"
    panel.mkdir()
    out = str(tmp_path / "out")
    for extra in ([], ["-i", "400"], ["--panelMetric", "weightedjaccard", "--panelRecursive"]):
        buf = io.StringIO()
        with redirect_stdout(buf):
            rc = main(["sketch", "-f", str(fq), "-o", out, "--panel", str(panel)] + extra)
        assert rc == 1
        assert buf.getvalue().rstrip().endswith("ERROR---> --panel needs --streamEvery")
        assert sorted(os.listdir(tmp_path)) == ["panel", "r.fq"], "nothing is written"


def test_cpp_panel_driver_compiles_and_links(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "panel_driver.cpp"), "-o", str(tmp_path / "panel_driver"),
           "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
