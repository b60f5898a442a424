"""What the banded index (hulk_index_*, tests/test_gpu_index.py) can be held to without a GPU: that its inputs exercise what they claim
(on the yardstick alone), the header's text, the binding's structs, the argument errors that come before any HIP call and the file
format's refusals — hulk_index_load reads, measures and checksums the file before it touches a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import index_inputs as ii
from conftest import ROOT

ERR_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_IO = -30, -31, -32, -35
ENTRY_POINTS = ("hulk_index_build", "hulk_index_search", "hulk_index_info", "hulk_index_free", "hulk_index_set_names", "hulk_index_name",
                "hulk_index_save", "hulk_index_load", "hulk_index_build_files", "hulk_index_search_files")


def test_header_declares_and_library_exports_the_entry_points():
    from hulk_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hulk_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in hulk_hip.h"
        assert hasattr(L, name), f"libhulkhip.so does not export {name}"
        assert name in _lib.ABI_SYMBOLS
    assert "#define HULK_ABI_VERSION 4" in hdr, "additions only: the ABI version stays"
    for struct in ("hulk_index_opts", "hulk_index_search_opts", "hulk_index_search_stats"):
        assert "typedef struct " + struct in code
    # the rule is stated where the other entry points state theirs
    for text in ("THEOREM", "u_max + 1", "1.0 - (double)(S - u) / (double)S <= D", "use hulk_search", "8 S + 20 B bytes", "returns synchronised",
                 "One call at a time per index"):
        assert text in " ".join(hdr.replace("\n *", " ").split()), text
    assert ctypes.sizeof(_lib.IndexOpts) == 56 and _lib.IndexOpts.reserved.offset == 24
    assert ctypes.sizeof(_lib.IndexSearchOpts) == 56 and _lib.IndexSearchOpts.max_distance.offset == 8
    assert ctypes.sizeof(_lib.IndexSearchStats) == 64 and _lib.IndexSearchStats.candidates.offset == 40


def test_the_rule_restated():
    assert ii.u_max(512, 0.1) == 51 and ii.default_bands(512, 0.1) == 52
    assert ii.u_max(33, 0.1) == 3 and ii.u_max(8, 0.0) == 0 and ii.u_max(8, 1.0) == 8
    assert ii.u_max(8, 0.25) == 2 and ii.u_max(8, np.nextafter(0.25, 0)) == 1
    assert ii.band_edges(33, 5) == [0, 6, 13, 19, 26, 33]
    # a key is a fold over the band in slot order: the order matters, the split does too
    m = np.array([[1, 2, 3, 4], [2, 1, 3, 4]], dtype=np.uint64)
    k1, k2 = ii.band_keys(m, 1), ii.band_keys(m, 2)
    assert k1[0, 0] != k1[1, 0] and k2[0, 0] != k2[1, 0] and k2[0, 1] == k2[1, 1]


@pytest.mark.parametrize("s", ii.THEOREM_SS)
def test_inputs_of_the_theorem(s):
    ii.check_theorem(s)
    cut, none = ii.check_self(s)
    print(f"S {s}: threshold {ii.theorem(s)[3]!r}, {ii.default_bands(s, ii.theorem(s)[3])} bands, {cut} lists cut by the limit, {none} queries without a candidate")
    ii.check_copies(s)


def test_inputs_of_the_planted_cases():
    for s, d in ii.PLANTED:
        ii.check_planted(s, d)
    ii.check_duplicates()
    ii.check_beyond_doubles()
    missed = ii.check_few_bands()
    print(f"2 bands at S 33: {missed} pairs within the threshold are no candidates")


def build(mins, **kw):
    from hulk_amd.smash import Index
    return Index.build(mins, **kw)


def test_build_errors_come_before_any_hip_call():
    """HULK_ERR_ARG with a text, on a machine with or without a device"""
    from hulk_amd import _lib
    from hulk_amd._lib import HulkError
    m = np.arange(32, dtype=np.uint64).reshape(4, 8)
    for kw, text in ((dict(max_distance=1.0), "every sketch is within this distance: use hulk_search"),
                     (dict(max_distance=-0.5), "max_distance must be in [0, 1)"), (dict(max_distance=float("nan")), "max_distance must be in [0, 1)"),
                     (dict(max_distance=1.5), "max_distance must be in [0, 1)"), (dict(max_distance=0.1, bands=9), "bands must be 0 (derived) or 1 .. sketch_size"),
                     (dict(max_distance=0.1, metric="weightedjaccard"), "weightedjaccard and bottomk cannot be indexed"),
                     (dict(max_distance=0.1, metric="bottomk"), "weightedjaccard and bottomk cannot be indexed")):
        with pytest.raises(HulkError) as e:
            build(m, **kw)
        assert e.value.code == ERR_ARG and text in e.value.message, (kw, e.value.message)
    L = _lib.load()
    h = ctypes.c_void_p()
    o = _lib.IndexOpts(max_distance=0.1)
    assert L.hulk_index_build(0, None, 4, 8, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG and b"NULL" in L.hulk_last_error(None)
    assert L.hulk_index_build(0, m.ctypes.data, 4, 8, None, ctypes.byref(h)) == ERR_ARG
    assert L.hulk_index_build(0, m.ctypes.data, 4, 8, ctypes.byref(o), None) == ERR_ARG
    assert L.hulk_index_build(0, m.ctypes.data, 0, 8, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG and b"positive" in L.hulk_last_error(None)
    o = _lib.IndexOpts(max_distance=0.1, flags=1)
    assert L.hulk_index_build(0, m.ctypes.data, 4, 8, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG and b"flags" in L.hulk_last_error(None)
    o = _lib.IndexOpts(max_distance=0.1); o.reserved[3] = 1
    assert L.hulk_index_build(0, m.ctypes.data, 4, 8, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG and b"reserved" in L.hulk_last_error(None)
    assert h.value is None
    so = _lib.IndexSearchOpts(k=1)
    out = np.zeros(8, dtype=np.uint64)
    assert L.hulk_index_search(None, m.ctypes.data, 4, ctypes.byref(so), out.ctypes.data, out.ctypes.data, out.ctypes.data, None) == ERR_ARG
    assert L.hulk_index_info(None, None, None, None, None, None) == ERR_ARG and L.hulk_index_name(None, 0) is None
    assert L.hulk_index_save(None, b"x") == ERR_ARG and L.hulk_index_load(0, None, ctypes.byref(h)) == ERR_ARG
    L.hulk_index_free(None)


def test_file_format_refusals(tmp_path):
    """a truncated, corrupt or foreign file is HULK_ERR_IO with a text before any HIP call; a well-formed one gets as far as the device"""
    from hulk_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(3)
    mins = rng.integers(0, 1 << 40, size=(5, 8)).astype(np.uint64)
    good = ii.index_file(mins, 0.25, 3, [f"s{i}.json" for i in range(5)])
    assert len(good) == 48 + 5 * 8 + 5 * 8 * 8 + 4

    def load(data):
        p = str(tmp_path / "x.hulk-index")
        with open(p, "wb") as fh:
            fh.write(data)
        h = ctypes.c_void_p()
        rc = L.hulk_index_load(0, p.encode(), ctypes.byref(h))
        msg = L.hulk_last_error(None).decode()
        if rc == 0:
            L.hulk_index_free(h)
        else:
            assert h.value is None, "a partly loaded index"
        return rc, msg
    rc, msg = load(good)
    assert rc in (0, ERR_NO_DEVICE, ERR_HIP), (rc, msg)                 # the file is accepted: what is left is the device's
    for cut in (0, 7, 47, 48, 60, len(good) - 5, len(good) - 1):
        rc, msg = load(good[:cut])
        assert rc == ERR_IO and "truncated" in msg, (cut, rc, msg)
    rc, msg = load(good + b"\0")
    assert rc == ERR_IO
    for at in (9, 13, 17, 21, 25, 33, 41, 50, 100, len(good) - 2):
        bad = bytearray(good); bad[at] ^= 0x10
        rc, msg = load(bytes(bad))
        assert rc == ERR_IO and msg, (at, rc, msg)
    rc, msg = load(b"{\"not\": \"an index\"}" + bytes(100))
    assert rc == ERR_IO and "not a hulk index file" in msg
    rc, msg = load(ii.index_file(mins, 0.25, 3, ["a"] * 5, version=2))
    assert rc == ERR_IO and "format version 2" in msg
    # lengths and checksum right, the content not: names, threshold, bands
    for data in (ii.index_file(mins, 0.25, 3, ["a"] * 4), ii.index_file(mins, 1.0, 3, ["a"] * 5), ii.index_file(mins, 0.25, 9, ["a"] * 5),
                 ii.index_file(mins, 0.25, 0, ["a"] * 5)):
        rc, msg = load(data)
        assert rc == ERR_IO and "corrupt" in msg, (rc, msg)
    h = ctypes.c_void_p()
    assert L.hulk_index_load(0, str(tmp_path / "missing").encode(), ctypes.byref(h)) == ERR_IO and b"cannot open" in L.hulk_last_error(None)


def test_the_launch_plan_on_the_host_under_sanitizers(tmp_path):
    """hulk_index_plan.h is HIP-free: the text hulk_index_search plans its launches with, in a stand-alone program, at 2^20 queries x 103
    bands, under 16 GiB of scratch on a dense collection, with queries of 2^26 and 2^32 - 2 candidates: every launch stays below HIP's
    2^32 threads, the blocks and pieces cover every candidate exactly once in query order"""
    exe = str(tmp_path / "index_plan_host")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan",      # (the runtimes inside the program: it is whole on its own)
                        "-I", os.path.join(ROOT, "hulk_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "index_plan_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stdout.count(": ok") == 8, r.stdout[-3000:] + r.stderr[-3000:]


def test_shapes_beyond_the_launch_limits_are_refused_before_any_hip_call():
    """n * bands must stay below 2^32 (k_index_keys runs a thread per sketch and band): HULK_ERR_ARG with a text; the mins are not read"""
    from hulk_amd import _lib
    L = _lib.load()
    m = np.zeros(8, dtype=np.uint64)
    h = ctypes.c_void_p()
    o = _lib.IndexOpts(max_distance=0.5, bands=65535)
    assert L.hulk_index_build(0, m.ctypes.data, 65538, 65535, ctypes.byref(o), ctypes.byref(h)) == ERR_ARG
    assert b"sketches x bands must be below 2^32" in L.hulk_last_error(None) and h.value is None


def test_inputs_of_the_second_staging_piece():
    """S = 512, n = m = 16,448: the database and the full set of queries each need a second piece of upload_rows' staging buffer,
    and the planted copies and near-copies sit on both sides of the border"""
    db = ii.stage_database()
    ii.check_stage_database(db)
    qm, plan = ii.stage_build_queries(db)
    D, cand = ii.check_stage_build(db, qm, plan)
    lists, n_cand, n_within = ii.expected(D, cand, ii.STAGE_K, ii.STAGE_D)
    assert n_within == 64 - len(ii.STAGE_FAR) == int(lists[2].sum()) and n_cand == n_within + len(ii.STAGE_FAR) // 2
    full, perm, want = ii.stage_full_queries(db)
    ii.check_stage_full(db, full, perm, want)
    del db, qm, D, cand, full, perm, want
