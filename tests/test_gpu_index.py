"""The banded index over a sketch collection on the GPU (hulk_index_*: k_index_keys, the build's sort, k_index_probe twice around
k_index_scan, k_index_verify, k_index_select).

Every output array is compared byte for byte with the yardstick of tests/index_inputs.py: hit_index, the bits of hit_distance,
hit_count — search_inputs.select over the yardstick's distances with the non-candidates of the numpy restatement masked out — and
stats.candidates / stats.within with the restatement's counts.  Where the theorem applies the result is compared with hulk_search
itself too."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import index_inputs as ii
import search_inputs as si
from conftest import ROOT
from test_gpu_search import assert_hits, cli, write_sketch

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_IO = -30, -35


def same_bytes(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def run(ix, qm, D, cand, k, limit, what, self_search=False, **kw):
    """one search of the index against the restatement: lists, candidates, within"""
    st = {}
    got = ix.search(None if self_search else qm, k, max_distance=limit, self_search=self_search, stats=st, **kw)
    lim = ix.info["max_distance"] if limit is None else limit
    want, n_cand, n_within = ii.expected(D, cand, k, lim, self_search)
    assert_hits(got, want, what)
    assert (st["candidates"], st["within"]) == (n_cand, n_within), (what, st, n_cand, n_within)
    return got, st


# ---- 1. the theorem ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ii.THEOREM_SS)
def test_theorem(s):
    """S = 8: ties everywhere, the index decides; S = 33: bands of unequal length.  Five queries against the first N sketches of the
    database, N = 1, a wave less one, a wave, a wave and one, 1100; k = 1, 33, 64; the build's limit and half of it: the index's lists
    are the yardstick's over the WHOLE database and hulk_search's, byte for byte"""
    from hulk_amd.smash import Index, search
    qm, dm, D, d, dkeys, qkeys = ii.theorem(s)
    cand = ii.check_theorem(s)
    ones_q, ones_d = np.ones(qm.shape), np.ones(dm.shape)
    for n in ii.THEOREM_NS:
        with Index.build(dm[:n], d) as ix:
            info = ix.info
            b = ii.default_bands(s, d)
            assert (info["n"], info["sketch_size"], info["bands"], info["max_distance"]) == (n, s, b, d)
            assert info["device_bytes"] == n * (8 * s + 20 * b)
            for lim in (d, d / 2, None):
                for k in ii.THEOREM_KS:
                    what = f"S {s} N {n} K {k} limit {lim}"
                    got, _ = run(ix, qm, D[:, :n], cand[:, :n], k, lim, what)
                    assert_hits(got, si.select(D[:, :n], k, max_distance=d if lim is None else lim), what + " (the whole database)")
                    if lim is not None:
                        assert same_bytes(got, search(qm, ones_q, dm[:n], ones_d[:n], k, "jaccard", max_distance=lim)), what + " (hulk_search)"


# ---- 2. pigeonhole at its edge ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,d", ii.PLANTED)
def test_pigeonhole_at_its_edge(s, d):
    """for every band b a sketch that differs from the query in u_max slots with b its only intact band: a hit; one that differs in
    u_max + 1 slots, one in every band: no candidate"""
    from hulk_amd.smash import Index
    q, db = ii.planted(s, d)
    D, cand = ii.check_planted(s, d)
    b = ii.default_bands(s, d)
    with Index.build(db, d) as ix:
        assert ix.info["bands"] == b
        got, st = run(ix, q, D, cand, 64, None, f"planted S {s}")
        assert got[2][0] == b and sorted(got[0][0, :b].tolist()) == list(range(b)) and st["candidates"] == b == st["within"]


# ---- 3. D = 0 ---------------------------------------------------------------------------------------------------------------------------
def test_exact_duplicates_at_distance_zero():
    from hulk_amd.smash import Index
    q, db = ii.duplicates()
    D, cand = ii.check_duplicates()
    with Index.build(db, 0.0) as ix:
        assert ix.info["bands"] == 1
        for k in (1, 64):
            got, _ = run(ix, q, D, cand, k, None, f"duplicates K {k}")
            assert_hits(got, si.select(D, k, max_distance=0.0), "duplicates (the whole database)")
            assert (got[1][~np.isnan(got[1])] == 0.0).all()


# ---- 4. runs and de-duplication ---------------------------------------------------------------------------------------------------------
def test_runs_and_deduplication():
    """1100 identical sketches: every band holds one run of 1100 and every pair shares every band — 1100 candidates a query, not
    1100 * B; then search_inputs' `copies`: a run of equal sketches inside a random database"""
    from hulk_amd.smash import Index
    q, db = ii.identical()
    d = 0.1
    with Index.build(db, d) as ix:
        assert ix.info["bands"] == ii.default_bands(33, d) > 1
        for k in (1, 33, 64):
            st = {}
            index, dist, count = ix.search(q, k, stats=st)
            assert st["candidates"] == len(q) * len(db) == st["within"]
            assert (index == np.arange(k, dtype=np.uint32)[None, :]).all() and (count == k).all() and (dist == 0.0).all()
        st = {}
        index, dist, count = ix.search(None, 64, self_search=True, stats=st)
        assert st["candidates"] == len(db) * (len(db) - 1)
        want = np.array([[j for j in range(66) if j != i][:64] for i in range(len(db))], dtype=np.uint32)
        assert np.array_equal(index, want) and (count == 64).all()
    for s in ii.THEOREM_SS:
        qm, dm, D, d, cand = ii.copies(s)
        ii.check_copies(s)
        with Index.build(dm, d) as ix:
            for k in (1, 64):
                got, _ = run(ix, qm, D, cand, k, None, f"copies S {s} K {k}")
                assert_hits(got, si.select(D, k, max_distance=d), f"copies S {s} K {k} (the whole database)")


# ---- 5. mins as doubles -----------------------------------------------------------------------------------------------------------------
def test_mins_are_compared_as_doubles():
    from hulk_amd.smash import Index, search
    q, db = ii.beyond_doubles()
    D = ii.check_beyond_doubles()
    with Index.build(db, 0.0) as ix:
        st = {}
        got = ix.search(q, 3, stats=st)
        assert_hits(got, si.select(D, 3, max_distance=0.0), "beyond doubles")
        assert got[0][0, :2].tolist() == [0, 1] and st["candidates"] == 2
        assert same_bytes(got, search(q, np.ones(q.shape), db, np.ones(db.shape), 3, "jaccard", max_distance=0.0))


# ---- 6. fewer bands: an LSH filter ------------------------------------------------------------------------------------------------------
def test_fewer_bands_give_the_candidate_restricted_lists():
    from hulk_amd.smash import Index
    dm, D, d, bands, cand = ii.few_bands()
    ii.check_few_bands()
    with Index.build(dm, d, bands=bands) as ix:
        assert ix.info["bands"] == bands
        got, _ = run(ix, None, D, cand, si.LONG_K, None, f"{bands} bands", self_search=True)
        full = si.select(D, si.LONG_K, max_distance=d, no_diagonal=True)
        assert not np.array_equal(got[2], full[2]), "the filter lost nothing: the case does not tell the two definitions apart"
        from hulk_amd._lib import HulkError
        with pytest.raises(HulkError) as e:
            ix.search(None, 1, max_distance=np.nextafter(d, 1), self_search=True)
        assert e.value.code == ERR_ARG and "above" in e.value.message
        assert "%.17g" % np.nextafter(d, 1) in e.value.message and "%.17g is above the %.17g" % (np.nextafter(d, 1), d) in e.value.message, e.value.message


# ---- 7. SELF and 8. the scratch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", ii.THEOREM_SS)
def test_self_search_and_scratch(s):
    """the database among itself at N = 1100 against the restatement and hulk_search's SELF; then a scratch of 64 candidates: several
    query blocks, queries in pieces, the same bytes"""
    from hulk_amd.smash import Index, search
    dm, D, d, dkeys, cand = ii.self_case(s)
    ii.check_self(s)
    k = si.LONG_K
    with Index.build(dm, d) as ix:
        got, st = run(ix, None, D, cand, k, None, f"self S {s}", self_search=True)
        assert (st["query_blocks"], st["pieces"]) == (1, 0), st
        assert_hits(got, si.select(D, k, max_distance=d, no_diagonal=True), f"self S {s} (the whole database)")
        assert same_bytes(got, search(dm, np.ones(dm.shape), None, None, k, "jaccard", max_distance=d, self_search=True))
        per_query = cand.sum(axis=1)
        cap = 64
        assert (per_query > 2 * cap).sum() >= 3 and (per_query == 0).any() and ((per_query[:-1] + per_query[1:]) <= cap).any(), \
            si.NO_TEST + "no query goes in three pieces, or no block holds several queries"
        small, st2 = run(ix, None, D, cand, k, None, f"self S {s}, a scratch of {cap} candidates", self_search=True, scratch_bytes=16 * cap)
        assert st2["query_blocks"] > 3 and st2["pieces"] >= 2 * int((per_query > cap).sum()), st2
        assert same_bytes(got, small)
        for kk in (1, 33):
            a, _ = run(ix, None, D, cand, kk, d / 2, f"self S {s} K {kk}", self_search=True, scratch_bytes=16 * cap)
            assert same_bytes(a, search(dm, np.ones(dm.shape), None, None, kk, "jaccard", max_distance=d / 2, self_search=True))


# ---- 9. save and load -------------------------------------------------------------------------------------------------------------------
def test_save_and_load(tmp_path):
    from hulk_amd.smash import Index
    from hulk_amd._lib import HulkError
    s = 33
    qm, dm, D, d, dkeys, qkeys = ii.theorem(s)
    cand = ii.check_theorem(s)
    names = [f"dir/sketch,{i}.json" for i in range(len(dm))]
    path = str(tmp_path / "db.hulk-index")
    with Index.build(dm, d, names=names) as ix:
        before = [ix.search(qm, k) for k in ii.THEOREM_KS] + [ix.search(None, 5, self_search=True)]
        ix.save(path)
        info = ix.info
    data = open(path, "rb").read()
    assert data == ii.index_file(dm, d, info["bands"], names), "the file is not what the header describes"
    with Index.load(path) as ix:
        assert ix.info == info and ix.names == names
        after = [ix.search(qm, k) for k in ii.THEOREM_KS] + [ix.search(None, 5, self_search=True)]
        run(ix, qm, D, cand, 64, None, "a loaded index")
    assert all(same_bytes(a, b) for a, b in zip(before, after))
    bad = str(tmp_path / "bad.hulk-index")
    for cut in (0, 20, 48, 1000, len(data) // 2, len(data) - 1):
        open(bad, "wb").write(data[:cut])
        with pytest.raises(HulkError) as e:
            Index.load(bad)
        assert e.value.code == ERR_IO and "truncated" in e.value.message, (cut, e.value.message)
    for at in (30, 60, len(data) // 2, len(data) - 1):
        flipped = bytearray(data); flipped[at] ^= 1
        open(bad, "wb").write(bytes(flipped))
        with pytest.raises(HulkError) as e:
            Index.load(bad)
        assert e.value.code == ERR_IO and "corrupt" in e.value.message, (at, e.value.message)


# ---- 10. argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from hulk_amd import _lib
    from hulk_amd._lib import HulkError
    from hulk_amd.smash import Index
    qm, dm, D, d, _, _ = ii.theorem(8)
    for kw, text in ((dict(max_distance=1.0), "every sketch is within this distance: use hulk_search"),
                     (dict(max_distance=d, metric="weightedjaccard"), "cannot be indexed"), (dict(max_distance=d, metric="bottomk"), "cannot be indexed"),
                     (dict(max_distance=d, bands=9), "bands must be")):
        with pytest.raises(HulkError) as e:
            Index.build(dm[:10], **kw)
        assert e.value.code == ERR_ARG and text in e.value.message
    with Index.build(dm[:10], d) as ix:
        for kw, text in ((dict(k=0), "k must be 1 .. 64"), (dict(k=65), "k must be 1 .. 64"), (dict(k=1, max_distance=np.nextafter(d, 1)), "is above the"),
                         (dict(k=1, max_distance=1.0), "is above the"), (dict(k=1, scratch_bytes=8), "too small")):
            with pytest.raises(HulkError) as e:
                ix.search(qm, **kw)
            assert e.value.code == ERR_ARG and text in e.value.message, e.value.message
        L = _lib.load()
        out = np.zeros(64, dtype=np.uint64)
        o = _lib.IndexSearchOpts(k=1)
        args = (out.ctypes.data, out.ctypes.data, out.ctypes.data, None)
        assert L.hulk_index_search(ix._h, None, 5, ctypes.byref(o), *args) == ERR_ARG and b"no queries" in L.hulk_last_error(None)
        assert L.hulk_index_search(ix._h, qm.ctypes.data, 5, None, *args) == ERR_ARG and b"NULL" in L.hulk_last_error(None)
        assert L.hulk_index_search(ix._h, qm.ctypes.data, 5, ctypes.byref(o), None, out.ctypes.data, out.ctypes.data, None) == ERR_ARG
        assert L.hulk_index_search(ix._h, qm.ctypes.data, 0, ctypes.byref(o), *args) == ERR_ARG and b"positive" in L.hulk_last_error(None)
        o = _lib.IndexSearchOpts(k=1, flags=_lib.HULK_SEARCH_SELF)
        assert L.hulk_index_search(ix._h, qm.ctypes.data, 5, ctypes.byref(o), *args) == ERR_ARG and b"takes no queries" in L.hulk_last_error(None)
        o = _lib.IndexSearchOpts(k=1, flags=2)
        assert L.hulk_index_search(ix._h, qm.ctypes.data, 5, ctypes.byref(o), *args) == ERR_ARG and b"flags" in L.hulk_last_error(None)
        o = _lib.IndexSearchOpts(k=1); o.reserved[0] = 1
        assert L.hulk_index_search(ix._h, qm.ctypes.data, 5, ctypes.byref(o), *args) == ERR_ARG and b"reserved" in L.hulk_last_error(None)
        with pytest.raises(HulkError) as e:
            ix.search(qm[:, :7], 1)
        assert "sketch length mismatch: 7 vs 8" in e.value.message
        assert ix.names == [""] * 10
        with pytest.raises(HulkError):
            Index.build(dm[:10], d, names=["a"] * 9)
    with pytest.raises(ValueError):
        ix.search(qm, 1)                                            # closed


# ---- 11. the file forms and the CLI -----------------------------------------------------------------------------------------------------
def test_file_forms_and_cli(tmp_path):
    """an index created from a directory of sketch files and searched with a directory of queries: the CSV is `search`'s for the same
    --maxDistance and --top, byte for byte — from the binding and from the command line (-j, the reference's spelling, included)"""
    from hulk_amd import smash
    from hulk_amd._lib import HulkError
    rng = np.random.default_rng(67)
    S = 50
    base = rng.integers(0, 194481, size=S).astype(np.uint64)
    n = 60
    mins = np.where(rng.random((n, S)) < rng.uniform(0.8, 1.0, size=(n, 1)), base, rng.integers(0, 194481, size=(n, S)).astype(np.uint64))
    weights = -rng.gamma(2.0, 1e-3, size=(n, S))
    qdir, ddir, sub = tmp_path / "q", tmp_path / "db", tmp_path / "db" / "more"
    for p in (qdir, ddir, sub):
        p.mkdir()
    qnames = ["q0.json", "q,1.json", "q2.json"]
    for i in range(n):
        where = qdir / qnames[i] if i < 3 else (sub if i % 5 == 0 else ddir) / f"s{i:02d}.json"
        write_sketch(str(where), mins[i], weights[i])
    dfiles = smash.collect_jsons(str(ddir), recursive=True)
    qfiles = [str(qdir / x) for x in qnames]
    assert len(dfiles) == n - 3
    D, K = 1 - 0.80, 30                                            # (what -j 0.80 means: not the double 0.2)
    ref = str(tmp_path / "ref.csv")
    _, d_order, r_index, r_dist, r_count = smash.search_files(qfiles, dfiles, K, max_distance=D, csv_path=ref)
    assert 0 < r_count.sum() < 3 * K, si.NO_TEST + "the limit cuts no list, or every one to nothing"
    out = str(tmp_path / "ix.csv")
    with smash.Index.build_files(dfiles, D) as ix:
        assert ix.names == d_order and ix.info["bands"] == ii.default_bands(S, D)
        st = {}
        q_order, index, dist, count = ix.search_files(qfiles, K, csv_path=out, stats=st)
        assert q_order == sorted(qfiles) and same_bytes((index, dist, count), (r_index, r_dist, r_count)) and st["within"] >= count.sum()
        ix.save(str(tmp_path / "lib.hulk-index"))
        with pytest.raises(HulkError) as e:
            smash.Index.build_files([str(tmp_path / "nothing.json")], D)
        assert e.value.code == ERR_ARG
    assert open(out).read() == open(ref).read()
    with smash.Index.build_files(dfiles[:1], D) as one:                                  # a set of one sketch is valid
        assert one.info["n"] == 1
    name = str(tmp_path / "cami")
    r = cli(["index", "-r", "create", "-n", name, "-j", "0.80", "-d", str(ddir), "--recursive"])
    assert r.returncode == 0 and "HULK INDEX!" in r.stdout and f"indexed {n - 3} sketches" in r.stdout, r.stdout + r.stderr
    assert open(name + ".hulk-index", "rb").read() == open(str(tmp_path / "lib.hulk-index"), "rb").read()
    r = cli(["index", "-r", "search", "-n", name, "-d", str(qdir), "--top", str(K), "-o", str(tmp_path / "cli")])
    assert r.returncode == 0 and "candidates" in r.stdout, r.stdout + r.stderr
    assert open(str(tmp_path / "cli") + ".hulk-search.csv").read() == open(ref).read()
    ref2 = str(tmp_path / "ref2.csv")
    smash.search_files(qfiles[:2], dfiles, 3, max_distance=0.1, csv_path=ref2)
    r = cli(["index", "-r", "search", "-n", name, "-d", qfiles[0], qfiles[1], "--top", "3", "--maxDistance", "0.1", "-o", str(tmp_path / "cli2")])
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(str(tmp_path / "cli2") + ".hulk-search.csv").read() == open(ref2).read()
    for args, text in ((["-r", "create", "-n", name, "-d", str(ddir)], "exactly one of"),
                       (["-r", "create", "-n", name, "-j", "0.8", "--maxDistance", "0.2", "-d", str(ddir)], "exactly one of"),
                       (["-r", "search", "-n", name, "-d", str(qdir), "--maxDistance", "0.5", "-o", str(tmp_path / "x")], "is above the"),
                       (["-r", "search", "-n", str(tmp_path / "none"), "-d", str(qdir), "-o", str(tmp_path / "x")], "cannot open")):
        r = cli(["index"] + args)
        assert r.returncode == 1 and text in r.stdout, (args, r.stdout + r.stderr)


# ---- 12. the C++ host -------------------------------------------------------------------------------------------------------------------
def test_cpp_host_matches_the_python_binding(tmp_path):
    """hulk::Index (include/hulk.hpp): Build, Search, Save, Load, Search again — the hits of the ctypes path, bit for bit"""
    from hulk_amd.smash import Index
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    exe = str(tmp_path / "index_driver")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "index_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    s = 33
    qm, dm, D, d, _, _ = ii.theorem(s)
    dm = dm[:300]

    def dump(path, mins):
        with open(path, "w") as fh:
            for a in mins:
                fh.write(" ".join(str(int(v)) for v in a) + "\n")
    qf, df = str(tmp_path / "q.txt"), str(tmp_path / "db.txt")
    dump(qf, qm); dump(df, dm)
    for self_search, k, bands, limit, scratch in ((False, 64, 0, -1.0, 0), (False, 5, 2, d / 2, 0), (True, 33, 0, -1.0, 16 * 64)):
        r = subprocess.run([exe, "-" if self_search else qf, df, str(s), str(k), repr(d), str(bands), repr(limit), str(scratch),
                            str(tmp_path / "cpp.hulk-index")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        st = {}
        with Index.build(dm, d, bands=bands) as ix:
            info = ix.info
            index, dist, count = ix.search(None if self_search else qm, k, max_distance=None if limit < 0 else limit, self_search=self_search,
                                           scratch_bytes=scratch, stats=st)
            ix.save(str(tmp_path / "py.hulk-index"))
        lines = r.stdout.strip().splitlines()
        assert lines[0] == f"info {info['n']} {info['sketch_size']} {info['bands']} {info['device_bytes']}"
        assert lines[-3] == f"stats {st['candidates']} {st['within']}" and lines[-2] == "loaded 1" and len(lines) == len(count) + 4
        assert lines[-1] == "empty -30", "an empty query list must be an argument error, not a self-join"
        for i, line in enumerate(lines[1:-3]):
            f = line.split()
            assert int(f[0]) == i and int(f[1]) == count[i] == len(f) - 2
            assert [int(x.split(":")[0]) for x in f[2:]] == index[i, :count[i]].tolist()
            assert [float.fromhex(x.split(":")[1]) for x in f[2:]] == dist[i, :count[i]].tolist()
        assert open(str(tmp_path / "cpp.hulk-index"), "rb").read() == open(str(tmp_path / "py.hulk-index"), "rb").read()
    r = subprocess.run([exe, qf, df, str(s), "5", "1.0", "0", "-1", "0", str(tmp_path / "x")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "hulk::Error -30|" in r.stdout and "use hulk_search" in r.stdout


# ---- the staging buffer's second piece ---------------------------------------------------------------------------------------------------
def test_build_in_two_staging_pieces():
    """S = 512, n = 16,448: upload_rows sends the database up in a piece of 16,384 sketches and one of 64, the second to d_out + 2^23.
    64 queries whose only hits are copies and near-copies of rows in both pieces, on either side of the border"""
    from hulk_amd.smash import Index, search
    db = ii.stage_database()
    ii.check_stage_database(db)
    qm, plan = ii.stage_build_queries(db)
    D, cand = ii.check_stage_build(db, qm, plan)
    with Index.build(db, ii.STAGE_D) as ix:
        assert (ix.info["n"], ix.info["sketch_size"], ix.info["bands"]) == (ii.STAGE_N, ii.STAGE_S, ii.default_bands(ii.STAGE_S, ii.STAGE_D))
        got, st = run(ix, qm, D, cand, ii.STAGE_K, None, "two pieces of the database")
        assert int(got[2].sum()) == 64 - len(ii.STAGE_FAR)
    ones = np.ones(db.shape)
    assert same_bytes(got, search(qm, ones[:64], db, ones, ii.STAGE_K, "jaccard", max_distance=ii.STAGE_D)), "hulk_search"
    del db, ones, D, cand


def test_queries_in_two_staging_pieces():
    """m = 16,448 queries at S = 512: the query side of upload_rows takes its second piece.  Query i is a copy (or a planted
    near-copy) of database row perm[i] and shares no slot with any other row: its list is known by construction"""
    from hulk_amd.smash import Index, search
    db = ii.stage_database()
    qm, perm, want = ii.stage_full_queries(db)
    ii.check_stage_full(db, qm, perm, want)
    with Index.build(db, ii.STAGE_D) as ix:
        st = {}
        got = ix.search(qm, ii.STAGE_K, stats=st)
    assert_hits(got, want, "two pieces of the queries")
    assert same_bytes(got, want)
    assert st["within"] == ii.STAGE_N - len(ii.STAGE_FAR) and st["candidates"] == st["within"] + len(ii.STAGE_FAR) // 2, st
    ones = np.ones(db.shape)
    assert same_bytes(got, search(qm, ones, db, ones, ii.STAGE_K, "jaccard", max_distance=ii.STAGE_D)), "hulk_search"
    del db, qm, ones
