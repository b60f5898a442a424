"""Single-linkage clustering (hulk_cluster, hulk_cluster_files), the parts that need no GPU: the header declares the entry points and
the built library exports them, every argument error is refused with its text before the library looks for a device, the CLI refuses
its bad flag combinations, the yardstick's own union-find is right on a hand-worked example, the generators of
tests/test_gpu_cluster.py produce inputs that test what they claim (tests/cluster_inputs.py, evaluated against oracle.pyorc), and
the kernel's union-find (hulk_amd/csrc/hulk_unionfind.h) compiled for the host agrees with a sequential one under
-fsanitize=address,undefined, run by several threads."""
import ctypes
import io
import os
import re
import subprocess
from contextlib import redirect_stdout

import numpy as np
import pytest

import cluster_inputs as ci
from conftest import ROOT

ENTRY_POINTS = ("hulk_cluster", "hulk_cluster_files")
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
    assert re.search(r"#define HULK_CLUSTER_MAX_N 2097088u\b", code) and _lib.HULK_CLUSTER_MAX_N == 2097088 == 65535 * 32 // 64 * 64
    assert "typedef struct hulk_cluster_opts" in code and "typedef struct hulk_cluster_stats" in code
    assert "#define HULK_ABI_VERSION 4" in hdr, "additions only: the ABI version stays"
    L.hulk_abi_version.restype = ctypes.c_int
    assert L.hulk_abi_version() == 4
    # the structs as the header lays them out
    assert ctypes.sizeof(_lib.ClusterOpts) == 56 and _lib.ClusterOpts.max_distance.offset == 8 and _lib.ClusterOpts.band_rows.offset == 16
    assert _lib.ClusterOpts.flags.offset == 20 and _lib.ClusterOpts.reserved.offset == 24
    assert ctypes.sizeof(_lib.ClusterStats) == 40 and _lib.ClusterStats.links.offset == 24 and _lib.ClusterStats.clusters.offset == 36
    if os.path.exists(_lib.EXP_LIB_PATH):
        X = ctypes.CDLL(_lib.EXP_LIB_PATH)
        assert all(hasattr(X, n) for n in ENTRY_POINTS)


def _call(L, _lib, *, metric=0, tau=0.5, band=0, flags=0, reserved=(0, 0, 0, 0), n=3, S=4, mins=True, weights=True, label=True, opts=True, tiny=False):
    size = 1 if tiny else max(n, 1)                                 # (tiny: the arrays of a refused call are never touched)
    m = np.arange(size * max(S, 1), dtype=np.uint64); w = np.ones(size * max(S, 1))
    lab = np.zeros(size, dtype=np.uint32)
    o = _lib.ClusterOpts(metric=metric, max_distance=tau, band_rows=band, flags=flags)
    for i, v in enumerate(reserved):
        o.reserved[i] = v
    rc = L.hulk_cluster(0, m.ctypes.data if mins else None, w.ctypes.data if weights else None, n, S, ctypes.byref(o) if opts else None,
                        lab.ctypes.data if label else None, None)
    return rc, L.hulk_last_error(None).decode()


def test_every_argument_error_is_refused_with_its_text_before_a_device_is_looked_for():
    """each of these returns HULK_ERR_ARG, not HULK_ERR_NO_DEVICE: here there is no device, and the argument checks come first"""
    from hulk_amd import _lib
    L = _lib.load()
    cases = [
        (dict(mins=False), "hulk_cluster: NULL"),
        (dict(weights=False), "hulk_cluster: NULL"),
        (dict(label=False), "hulk_cluster: NULL"),
        (dict(opts=False), "hulk_cluster: NULL"),
        (dict(n=0), "n and sketch_size must be positive"),
        (dict(S=0), "n and sketch_size must be positive"),
        (dict(n=_lib.HULK_CLUSTER_MAX_N + 1, S=1), "n must be at most 2097088"),      # (the preparation is one launch: its grid.y)
        (dict(n=2 ** 32 - 1, S=1, tiny=True), "n must be at most 2097088"),
        (dict(metric=2), "hulk_cluster: metric"),
        (dict(metric=-1), "hulk_cluster: metric"),
        (dict(tau=-0.25), "max_distance must be in [0, 1]"),
        (dict(tau=1.0000000000000002), "max_distance must be in [0, 1]"),
        (dict(tau=float("nan")), "max_distance must be in [0, 1]"),
        (dict(tau=float("inf")), "max_distance must be in [0, 1]"),
        (dict(band=1), "band_rows must be a multiple of 32"),
        (dict(band=48), "band_rows must be a multiple of 32"),
        (dict(flags=1), "unknown flags"),
        (dict(reserved=(0, 0, 0, 1)), "reserved fields must be zero"),
        (dict(reserved=(7, 0, 0, 0)), "reserved fields must be zero"),
    ]
    for kw, text in cases:
        rc, msg = _call(L, _lib, **kw)
        assert rc == ERR_ARG and text in msg, (kw, rc, msg)
    # what is valid gets past the argument checks (and then finds no device here, or runs): the ends of [0, 1], -0.0, one sketch
    for kw in (dict(tau=0.0), dict(tau=-0.0), dict(tau=1.0), dict(n=1), dict(band=32), dict(band=96), dict(metric=1)):
        rc, msg = _call(L, _lib, **kw)
        assert rc in (0, ERR_NO_DEVICE), (kw, rc, msg)


def test_python_binding_refuses_without_a_device():
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    rng = np.random.default_rng(1)
    m = rng.integers(0, 100, size=(3, 8)).astype(np.uint64); w = -rng.random((3, 8))
    for tau in (-0.1, 1.5, float("nan")):
        with pytest.raises(HulkError, match=r"max_distance must be in \[0, 1\]") as ei:
            smash.cluster(m, w, tau)
        assert ei.value.code == ERR_ARG
    with pytest.raises(HulkError, match="band_rows must be a multiple of 32"):
        smash.cluster(m, w, 0.5, band_rows=33)
    with pytest.raises(HulkError, match="supplied distance metric is not available: cosine"):
        smash.cluster(m, w, 0.5, metric="cosine")
    with pytest.raises(ValueError):
        smash.cluster(m, w[:, :7], 0.5)
    with pytest.raises(HulkError, match="supplied algorithm not available: minhash"):
        smash.cluster_files(["a.json"], 0.5, algo="minhash")
    with pytest.raises(HulkError, match=r"max_distance must be in \[0, 1\]"):
        smash.cluster_files(["a.json"], 2.0)
    with pytest.raises(HulkError) as ei:
        smash.cluster_files([], 0.5)
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
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    db = _sketch_files(tmp_path, 3, 16)
    for files in (db, db[:1]):                                      # a set of one sketch is valid: loading is all that can succeed here
        try:
            smash.cluster_files(files, 0.5)
        except HulkError as e:
            assert e.code == ERR_NO_DEVICE, (e.code, e.message)
    bad = str(tmp_path / "bad.json")
    open(bad, "w").write(open(db[0]).read().replace('"mins": [', '"mins": [1, ', 1))
    with pytest.raises(HulkError) as ei:
        smash.cluster_files(db + [bad], 0.5)
    assert ei.value.code == ERR_ARG and re.fullmatch(r"md5sum mismatch: [0-9a-f]{32} vs\. [0-9a-f]{32}\n", ei.value.message), ei.value.message
    short = _sketch_files(tmp_path, 1, 12, seed=5, prefix="s")
    with pytest.raises(HulkError) as ei:
        smash.cluster_files(db + short, 0.5)
    assert ei.value.message == "sketch length mismatch: 16 vs 12\n"
    with pytest.raises(HulkError, match=r"specified k-mer size \(15\) not found"):
        smash.cluster_files(db, 0.5, ksize=15)
    with pytest.raises(HulkError, match="no sketches were produced using the kmv algorithm"):
        smash.cluster_files(db, 0.5, algo="kmv")


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
             (["--maxDistance", "0.1", "-m", "cosine"], "supplied distance metric is not available: cosine"),
             (["--maxDistance", "0.1", "-a", "minhash"], "supplied algorithm not available: minhash\nplease select one of the following: ['histosketch', 'kmv', 'khf']"))
    for extra, text in cases:
        buf = io.StringIO()
        with redirect_stdout(buf):
            rc = main(["cluster", "-d", str(db), "-o", out] + extra)
        assert rc == 1, (extra, buf.getvalue())
        assert "ERROR---> " + text in buf.getvalue(), buf.getvalue()
        assert sorted(os.listdir(tmp_path)) == ["db"], "nothing is written"


def test_the_yardsticks_union_find_on_a_hand_worked_example():
    # 0-3, 3-5 | 1-2 | 4 | 6-7 given as 7-6: labels are the smallest members whatever the order and direction of the edges
    want = [0, 1, 1, 0, 4, 0, 6, 6]
    for edges in ([(0, 3), (3, 5), (1, 2), (7, 6)], [(5, 3), (7, 6), (2, 1), (3, 0)], [(7, 6), (5, 3), (3, 0), (1, 2), (0, 5), (2, 2)]):
        assert ci.union_find_labels(8, edges).tolist() == want
    assert ci.union_find_labels(1, []).tolist() == [0]
    # the rule on a 4 x 4 matrix: (0, 1) holds in one direction only, (2, 3) at exactly tau, NaN never links
    nan = float("nan")
    D = np.array([[0.0, 0.2, 0.9, nan],
                  [0.8, 0.0, 0.9, nan],
                  [0.9, 0.9, nan, 0.5],
                  [nan, nan, 0.5, 0.0]])
    labels, links, clusters = ci.components(D, 0.5)
    assert labels.tolist() == [0, 0, 2, 2] and links == 3 and clusters == 2
    labels, links, clusters = ci.components(D, 0.5, rule="and")
    assert labels.tolist() == [0, 1, 2, 2] and clusters == 3
    assert ci.components(D, np.nextafter(0.5, 0.0))[0].tolist() == [0, 0, 2, 3]
    assert ci.is_bridge(D, 0.5, (0, 1)) and ci.is_bridge(D, 0.5, (3, 2)) and not ci.is_bridge(D, 0.5, (0, 2))
    labels, links, clusters = ci.components(D, 1.0)
    assert labels.tolist() == [0, 0, 0, 0] and links == 8 and clusters == 1
    assert [ci.bands_planned(257, b) for b in ci.BANDS] == [1, 9, 3]


@pytest.mark.parametrize("s", [8, 33, 512])
def test_planted_chains_are_a_test(s):
    tau, (labels, links, clusters) = ci.check_planted_chains(s)
    print(f"S {s}: tau {tau!r}, {links} links, {clusters} clusters, sizes {sorted(np.bincount(labels)[np.bincount(labels) > 1].tolist())}")


def test_the_other_generators_are_a_test():
    for order in ("ascending", "descending", "random"):
        ci.check_ordered_chain(order)
    got = ci.check_weighted_set()
    print({t: (v[1], v[2]) for t, v in got.items()})
    for s in (1, 8, 33):
        ci.check_random_set(s)
    for s in (1, 8, 33, 512):
        _, _, plan = ci.shapes_plan(s)
        print({m: (t, ci.components(D, t)[1:]) for m, (D, t) in plan.items()})


def test_the_kernels_union_find_on_host_threads_under_sanitizers(tmp_path):
    """hulk_unionfind.h is HIP-free: the same text, with the two atomics mapped to the host compiler's builtins, in a stand-alone
    program that unites random and chain-shaped edge lists from 8 threads and compares with a sequential union-find"""
    exe = str(tmp_path / "unionfind_host")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan",      # (the runtimes inside the program: it is whole on its own)
                        "-I", os.path.join(ROOT, "hulk_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "unionfind_host.cpp"), "-o", exe, "-lpthread"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stdout.count(": ok") == 12, r.stdout + r.stderr[-3000:]


def test_cpp_cluster_driver_compiles_and_links(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "cluster_driver.cpp"), "-o", str(tmp_path / "cluster_driver"),
           "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
