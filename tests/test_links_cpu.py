"""The sparse link list (hulk_links, hulk_links_files), the parts that need no GPU: the header declares the entry points and the built
library exports them, the two structs are laid out as the header lays them out, every argument error is refused with its text before
the library looks for a device, the list functions take NULL, the CLI refuses its bad flag combinations, the yardstick
(tests/links_inputs.py) is right on a hand-worked example and the inputs of tests/test_gpu_links.py test what they claim, the
placement arithmetic the kernels share (hulk_amd/csrc/hulk_links_place.h) compiled for the host hits every slot exactly once in
ascending column order under -fsanitize=address,undefined, and the C++ driver compiles and links."""
import ctypes
import io
import os
import re
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

import bottomk_inputs as bi
import cluster_inputs as ci
import links_inputs as li
from conftest import ROOT

ENTRY_POINTS = ("hulk_links", "hulk_links_files")
LIST_FUNCTIONS = ("hulk_link_list_info", "hulk_link_list_row_start", "hulk_link_list_cols", "hulk_link_list_distances", "hulk_link_list_free")
ERR_ARG, ERR_NO_DEVICE = -30, -32


def test_header_declares_and_library_exports_the_entry_points():
    from hulk_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hulk_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(int device" % name, code), f"{name} is not declared in hulk_hip.h"
    for name in ENTRY_POINTS + LIST_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in hulk_hip.h"
        assert hasattr(L, name), f"libhulkhip.so does not export {name}"
        assert name in _lib.ABI_SYMBOLS
    assert re.search(r"#define HULK_LINKS_UPPER 1u\b", code) and _lib.HULK_LINKS_UPPER == 1
    assert "#define HULK_ABI_VERSION 4" in hdr, "additions only: the ABI version stays"
    L.hulk_abi_version.restype = ctypes.c_int
    assert L.hulk_abi_version() == 4
    if os.path.exists(_lib.EXP_LIB_PATH):
        X = ctypes.CDLL(_lib.EXP_LIB_PATH)
        assert all(hasattr(X, n) for n in ENTRY_POINTS + LIST_FUNCTIONS)


def test_struct_sizes_and_offsets_against_the_header(tmp_path):
    """the compiler's sizeof / offsetof of the two structs, printed by a program that includes the header, against ctypes'"""
    from hulk_amd import _lib
    fields = {"hulk_links_opts": ("metric", "max_distance", "band_rows", "flags", "max_edges", "reserved"),
              "hulk_links_stats": ("seconds_total", "kernel_ms_count", "kernel_ms_fill", "edges", "bands", "max_degree")}
    src = tmp_path / "layout.cpp"
    body = "".join(f'    printf("{s} %zu", sizeof({s}));\n' + "".join(f'    printf(" %zu", offsetof({s}, {f}));\n' for f in fs) + '    printf("\\n");\n'
                   for s, fs in fields.items())
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hulk_hip.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.strip().splitlines()
    for line, (name, cls) in zip(out, (("hulk_links_opts", _lib.LinksOpts), ("hulk_links_stats", _lib.LinksStats))):
        tok = line.split()
        assert tok[0] == name and int(tok[1]) == ctypes.sizeof(cls), (line, ctypes.sizeof(cls))
        assert [int(x) for x in tok[2:]] == [getattr(cls, f).offset for f in fields[name]], (line, name)
        assert [f for f, _ in cls._fields_] == list(fields[name])
    assert ctypes.sizeof(_lib.LinksOpts) == 64 and _lib.LinksOpts.max_edges.offset == 24 and _lib.LinksOpts.reserved.offset == 32
    assert ctypes.sizeof(_lib.LinksStats) == 40 and _lib.LinksStats.edges.offset == 24 and _lib.LinksStats.max_degree.offset == 36


def _call(L, _lib, *, metric=0, tau=0.5, band=0, flags=0, max_edges=0, reserved=(0, 0, 0, 0), n=3, S=4, mins=True, weights=True, out=True, opts=True, tiny=False):
    size = 1 if tiny else max(n, 1)                                 # (tiny: the arrays of a refused call are never touched)
    m = np.arange(size * max(S, 1), dtype=np.uint64); w = np.ones(size * max(S, 1))
    o = _lib.LinksOpts(metric=metric, max_distance=tau, band_rows=band, flags=flags, max_edges=max_edges)
    for i, v in enumerate(reserved):
        o.reserved[i] = v
    handle = ctypes.c_void_p(0x1234)                                # (a refused call sets it to NULL)
    st = _lib.LinksStats(edges=77)
    rc = L.hulk_links(0, m.ctypes.data if mins else None, w.ctypes.data if weights else None, n, S, ctypes.byref(o) if opts else None,
                      ctypes.byref(handle) if out else None, ctypes.byref(st))
    msg = L.hulk_last_error(None).decode()
    if rc == 0:
        L.hulk_link_list_free(handle)
    else:
        assert not out or handle.value is None, "a failed call leaves *out NULL"
        assert st.edges == 0
    return rc, msg


def test_every_argument_error_is_refused_with_its_text_before_a_device_is_looked_for():
    """each of these returns HULK_ERR_ARG, not HULK_ERR_NO_DEVICE: here there is no device, and the argument checks come first"""
    from hulk_amd import _lib
    L = _lib.load()
    cases = [
        (dict(mins=False), "hulk_links: NULL"),
        (dict(weights=False), "hulk_links: NULL"),
        (dict(weights=False, metric=1), "hulk_links: NULL"),
        (dict(out=False), "hulk_links: NULL"),
        (dict(opts=False), "hulk_links: NULL"),
        (dict(n=0), "n and sketch_size must be positive"),
        (dict(S=0), "n and sketch_size must be positive"),
        (dict(n=_lib.HULK_CLUSTER_MAX_N + 1, S=1), "n must be at most 2097088"),
        (dict(n=2 ** 32 - 1, S=1, tiny=True), "n must be at most 2097088"),
        (dict(metric=2), "hulk_links: metric"),
        (dict(metric=-1), "hulk_links: metric"),
        (dict(metric=4), "hulk_links: metric"),
        (dict(metric=3, S=_lib.HULK_MINHASH_MAX_SKETCH + 1, n=1), "bottomk takes a sketch_size of at most 4096"),
        (dict(tau=-0.25), "max_distance must be in [0, 1]"),
        (dict(tau=1.0000000000000002), "max_distance must be in [0, 1]"),
        (dict(tau=float("nan")), "max_distance must be in [0, 1]"),
        (dict(tau=float("inf")), "max_distance must be in [0, 1]"),
        (dict(band=1), "band_rows must be a multiple of 32"),
        (dict(band=48), "band_rows must be a multiple of 32"),
        (dict(flags=2), "unknown flags"),
        (dict(flags=3), "unknown flags"),
        (dict(flags=1 << 31), "unknown flags"),
        (dict(reserved=(0, 0, 0, 1)), "reserved fields must be zero"),
        (dict(reserved=(7, 0, 0, 0)), "reserved fields must be zero"),
    ]
    for kw, text in cases:
        rc, msg = _call(L, _lib, **kw)
        assert rc == ERR_ARG and text in msg, (kw, rc, msg)
    # what is valid gets past the argument checks (and then finds no device here, or runs): the ends of [0, 1], -0.0, one sketch,
    # the upper flag, a cap, bottomk without weights
    for kw in (dict(tau=0.0), dict(tau=-0.0), dict(tau=1.0), dict(n=1), dict(band=32), dict(band=96), dict(metric=1), dict(flags=1),
               dict(max_edges=1), dict(max_edges=2 ** 64 - 1), dict(metric=3, weights=False), dict(metric=3, S=_lib.HULK_MINHASH_MAX_SKETCH, n=1)):
        rc, msg = _call(L, _lib, **kw)
        assert rc in (0, ERR_NO_DEVICE), (kw, rc, msg)


def test_list_functions_take_null():
    from hulk_amd import _lib
    L = _lib.load()
    L.hulk_link_list_free(None)
    n, edges = ctypes.c_uint32(5), ctypes.c_uint64(6)
    assert L.hulk_link_list_info(None, ctypes.byref(n), ctypes.byref(edges)) == ERR_ARG and (n.value, edges.value) == (5, 6)
    assert L.hulk_link_list_row_start(None) is None and L.hulk_link_list_cols(None) is None and L.hulk_link_list_distances(None) is None


def test_python_binding_refuses_without_a_device():
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    rng = np.random.default_rng(1)
    m = rng.integers(0, 100, size=(3, 8)).astype(np.uint64); w = -rng.random((3, 8))
    for tau in (-0.1, 1.5, float("nan")):
        with pytest.raises(HulkError, match=r"max_distance must be in \[0, 1\]") as ei:
            smash.links(m, w, tau)
        assert ei.value.code == ERR_ARG
    with pytest.raises(HulkError, match="band_rows must be a multiple of 32"):
        smash.links(m, w, 0.5, band_rows=33)
    with pytest.raises(HulkError, match="supplied distance metric is not available: euclidean"):
        smash.links(m, w, 0.5, metric="euclidean")
    with pytest.raises(ValueError):
        smash.links(m, w[:, :7], 0.5)
    with pytest.raises(ValueError):
        smash.links(m, w, 0.5, max_edges=-1)
    with pytest.raises(HulkError, match="supplied algorithm not available: minhash"):
        smash.links_files(["a.json"], 0.5, algo="minhash")
    with pytest.raises(HulkError, match=r"max_distance must be in \[0, 1\]"):
        smash.links_files(["a.json"], 2.0)
    with pytest.raises(HulkError) as ei:
        smash.links_files([], 0.5)
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


def test_directory_form_loads_one_sketch_and_reports_the_reference_texts(tmp_path):
    """hulk_cluster_files' loader, texts and order"""
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    db = _sketch_files(tmp_path, 3, 16)
    for files in (db, db[:1]):                                      # a set of one sketch is valid: loading is all that can succeed here
        try:
            smash.links_files(files, 0.5)
        except HulkError as e:
            assert e.code == ERR_NO_DEVICE, (e.code, e.message)
    bad = str(tmp_path / "bad.json")
    open(bad, "w").write(open(db[0]).read().replace('"mins": [', '"mins": [1, ', 1))
    with pytest.raises(HulkError) as ei:
        smash.links_files(db + [bad], 0.5)
    assert ei.value.code == ERR_ARG and re.fullmatch(r"md5sum mismatch: [0-9a-f]{32} vs\. [0-9a-f]{32}\n", ei.value.message), ei.value.message
    short = _sketch_files(tmp_path, 1, 12, seed=5, prefix="s")
    with pytest.raises(HulkError) as ei:
        smash.links_files(db + short, 0.5)
    assert ei.value.message == "sketch length mismatch: 16 vs 12\n"
    with pytest.raises(HulkError, match=r"specified k-mer size \(15\) not found"):
        smash.links_files(db, 0.5, ksize=15)
    with pytest.raises(HulkError, match="no sketches were produced using the kmv algorithm"):
        smash.links_files(db, 0.5, algo="kmv")
    with pytest.raises(HulkError, match="bottomk is only supported for kmv sketches"):
        smash.links_files(db, 0.5, metric="bottomk")


def test_cli_refuses_bad_flags(tmp_path):
    from hulk_amd.__main__ import main
    db = tmp_path / "db"
    db.mkdir()
    _sketch_files(db, 2, 8)
    out = str(tmp_path / "out")
    cases = ((["--maxDistance", "0.1", "--minSimilarity", "90"], "exactly one of --maxDistance and --minSimilarity is required"),
             ([], "exactly one of --maxDistance and --minSimilarity is required"),
             (["--maxDistance", "1.5"], "--maxDistance must be between 0 and 1"),
             (["--maxDistance", "-0.5"], "--maxDistance must be between 0 and 1"),
             (["--maxDistance", "nan"], "--maxDistance must be between 0 and 1"),
             (["--minSimilarity", "101"], "--minSimilarity must be between 0 and 100"),
             (["--minSimilarity", "-1"], "--minSimilarity must be between 0 and 100"),
             (["--maxDistance", "0.1", "--maxEdges", "-3"], "--maxEdges must not be negative"),
             (["--maxDistance", "0.1", "-m", "cosine"], "supplied distance metric is not available: cosine"),
             (["--maxDistance", "0.1", "-a", "minhash"], "supplied algorithm not available: minhash\nplease select one of the following: ['histosketch', 'kmv', 'khf']"))
    for extra, text in cases:
        buf = io.StringIO()
        with redirect_stdout(buf):
            rc = main(["links", "-d", str(db), "-o", out] + extra)
        assert rc == 1, (extra, buf.getvalue())
        assert "ERROR---> " + text in buf.getvalue(), buf.getvalue()
        assert sorted(os.listdir(tmp_path)) == ["db"], "nothing is written"


def test_the_yardstick_on_a_hand_worked_example():
    nan = float("nan")
    D = np.array([[0.0, 0.2, 0.9, nan],
                  [0.8, 0.0, 0.5, nan],
                  [0.9, 0.9, nan, 0.5],
                  [nan, 0.1, 0.5, 0.0]])
    ptr, idx, dist = li.csr(D, 0.5)
    assert ptr.tolist() == [0, 1, 2, 3, 5] and idx.tolist() == [1, 2, 3, 1, 2] and dist.tolist() == [0.2, 0.5, 0.5, 0.1, 0.5]
    assert int(ptr[-1]) == ci.components(D, 0.5)[1], "edges is the clustering's links"
    up = li.csr(D, 0.5, upper=True)
    assert up[0].tolist() == [0, 1, 2, 3, 3] and up[1].tolist() == [1, 2, 3]
    li.assert_same(li.upper_of(ptr, idx, dist), up, "upper_of")
    assert li.csr(D, np.nextafter(0.5, 0.0))[1].tolist() == [1, 1]
    assert li.csr(D, 1.0)[0].tolist() == [0, 2, 4, 7, 9], "a NaN is never listed, the diagonal neither"
    one = li.csr(np.zeros((1, 1)), 1.0)
    assert one[0].tolist() == [0, 0] and len(one[1]) == 0 and len(one[2]) == 0
    assert li.render_csv(["a,b", "c"], (np.array([0, 1, 1], np.uint64), np.array([1], np.uint32), np.array([0.25]))) == \
        'sketch,neighbour,distance,similarity\n"a,b",c,0.25,75.00\n'


@pytest.mark.parametrize("s", [8, 33, 512])
def test_planted_chains_are_a_test_of_the_links(s):
    tau = li.check_chain_links(s)
    print(f"S {s}: tau {tau!r}")


def test_the_other_inputs_are_a_test_of_the_links():
    out = li.check_weighted_links()
    print({t: int(v[0][-1]) for t, v in out.items()})
    for s in (1, 8, 33):
        li.check_random_links(s)
    # bottomk: the planted set's matrix is the multiset yardstick's own; something links at 0.5 and not everything does
    mins = bi.planted_set(70, 40)
    D = bi.matrix(mins)
    e = int(li.csr(D, 0.5)[0][-1])
    assert 0 < e < 70 * 69, li.NO_TEST + f"bottomk: {e} links"
    assert np.array_equal(D, D.T), "bottomk is symmetric"


def test_the_placement_header_on_the_host_under_sanitizers(tmp_path):
    """hulk_links_place.h is HIP-free: the same text in a stand-alone program that restates the three kernels around it and runs
    them over all-zero, all-one, single-bit and random masks, with and without tiles in front that nobody reads"""
    exe = str(tmp_path / "links_place_host")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan",      # (the runtimes inside the program: it is whole on its own)
                        "-I", os.path.join(ROOT, "hulk_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "links_place_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stdout.count(": ok") == 1 + 7 * 9, r.stdout[-3000:] + r.stderr[-3000:]


def test_cpp_links_driver_compiles_and_links(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "links_driver.cpp"), "-o", str(tmp_path / "links_driver"),
           "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
