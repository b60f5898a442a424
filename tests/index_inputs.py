"""The yardstick of the index tests (tests/test_gpu_index.py, tests/test_index_cpu.py) and their inputs; no test lives here.

Distances and hit lists come from search_inputs.blocks / select (oracle.pyorc.smash_matrix, then the selection in numpy).  Beside them
stands a numpy restatement of the header's rule: u_max and the band edges, the band keys (a fold of oracle.pyorc.hash64 over the bits
of (double)min) and the candidate sets — sketch p is a candidate of query q when some band's keys are equal.  The expected result of an
index search is select() over the distances with every non-candidate masked out; stats.candidates and stats.within are the
restatement's counts.  With the default bands the theorem says the mask changes nothing: the tests compare with the unmasked lists too.
Every check_* function asserts on the yardstick alone that an input exercises what it claims ("the inputs are no test")."""
import functools
import struct
import zlib

import numpy as np

import search_inputs as si
from oracle import pyorc
from search_inputs import NO_TEST, NONE, frozen, select          # noqa: F401

MASK = 0xFFFFFFFFFFFFFFFF
THEOREM_SS = (8, 33)
THEOREM_NS = (1, 63, 64, 65, 1100)
THEOREM_KS = (1, 33, 64)
PLANTED = ((33, 0.1), (512, 0.1))


# ---- the rule, restated ----------------------------------------------------------------------------------------------------------------
def u_max(s, d):
    """the largest u in [0, s] with 1.0 - (double)(s - u) / (double)s <= d"""
    u = 0
    while u < s and 1.0 - (float(s - (u + 1)) / float(s)) <= d:
        u += 1
    return u


def default_bands(s, d):
    return u_max(s, d) + 1


def band_edges(s, b):
    return [i * s // b for i in range(b + 1)]


def band_keys(mins, b):
    """[n][b] uint64: h = 0, then h = hash64(h ^ bits((double)min[t]), ~0) over the band's slots in ascending order"""
    mins = np.ascontiguousarray(mins, dtype=np.uint64)
    n, s = mins.shape
    as_bits = mins.astype(np.float64).view(np.uint64)
    edges = band_edges(s, b)
    out = np.zeros((n, b), dtype=np.uint64)
    for i in range(n):
        row = as_bits[i].tolist()
        for j in range(b):
            h = 0
            for t in range(edges[j], edges[j + 1]):
                h = pyorc.hash64(h ^ row[t], MASK)
            out[i, j] = h
    return out


def candidates(qkeys, dkeys, self_search=False):
    """[m][n] bool: some band's keys are equal"""
    c = (qkeys[:, None, :] == dkeys[None, :, :]).any(axis=2)
    if self_search:
        c[np.arange(len(c)), np.arange(len(c))] = False
    return c


def expected(D, cand, k, limit, self_search=False):
    """(the lists over the candidates only, candidates, within): what an index search returns, from the yardstick's distances"""
    masked = np.where(cand, D, np.nan)
    lists = select(masked, k, max_distance=limit, no_diagonal=self_search)
    ok = cand & (D <= limit)
    return lists, int(cand.sum()), int(ok.sum())


def jaccard_blocks(qm, dm):
    """the yardstick's distances [m][n] under jaccard (weights play no part: ones)"""
    return si.blocks_few_queries(qm, np.ones(qm.shape), dm, np.ones(dm.shape), "jaccard")["row"]


# ---- 1. the theorem: long_inputs over a shared base -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def theorem(s):
    """(qm, dm, D [5][1100], the build threshold, db keys, query keys): the threshold leaves about 2 % of the database's own pairs
    within it (search_inputs.self_limit)"""
    qm, _, dm, _ = si.long_inputs(s)
    D = si.long_blocks(s, "jaccard")["row"]
    d = si.self_limit(s, "jaccard", "row")
    b = default_bands(s, d)
    return qm, dm, D, d, frozen(band_keys(dm, b))[0], frozen(band_keys(qm, b))[0]


def check_theorem(s):
    qm, dm, D, d, dkeys, qkeys = theorem(s)
    assert 0 < d < 1 and 1 < default_bands(s, d) <= s
    if s == 33:
        edges = band_edges(s, default_bands(s, d))
        assert len({edges[i + 1] - edges[i] for i in range(len(edges) - 1)}) > 1, NO_TEST + "the bands are of one length"
    cand = candidates(qkeys, dkeys)
    # the theorem on the yardstick: every pair within the threshold is a candidate
    assert not ((D <= d) & ~cand).any()
    assert ((D > d) & cand).any(), NO_TEST + "every candidate is a hit: the verification decides nothing"
    for n in THEOREM_NS:
        for lim in (d, d / 2):
            for k in THEOREM_KS:
                a = expected(D[:, :n], cand[:, :n], k, lim)[0]
                b = select(D[:, :n], k, max_distance=lim)
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    return cand


@functools.lru_cache(maxsize=None)
def self_case(s):
    """(dm, D [1100][1100], threshold, keys, candidates) of the database searched among itself"""
    _, dm, _, d, dkeys, _ = theorem(s)
    D = si.self_blocks(s, "jaccard")["row"]
    cand = candidates(dkeys, dkeys, self_search=True)
    return dm, D, d, dkeys, frozen(cand)[0]


def check_self(s):
    dm, D, d, dkeys, cand = self_case(s)
    off = ~np.eye(len(D), dtype=bool)
    assert not ((D <= d) & off & ~cand).any()
    index, dist, count = select(D, si.LONG_K, max_distance=d, no_diagonal=True)
    cut = int(((count > 0) & (count < si.LONG_K)).sum())
    assert cut >= 100, NO_TEST + f"{cut} lists are cut by the limit and not by k"
    none = int((cand.sum(axis=1) == 0).sum())
    assert none >= 1, NO_TEST + "every query has a candidate"
    return cut, none


# ---- 2. pigeonhole at its edge ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted(s, d):
    """(query [1][s], database [B + 1 + 8][s]): sketch b < B differs from the query in exactly u_max slots, one in every band but b;
    sketch B differs in u_max + 1 slots, one in every band; eight unrelated sketches follow"""
    rng = np.random.default_rng(7700 + s)
    u, b = u_max(s, d), default_bands(s, d)
    edges = band_edges(s, b)
    q = rng.choice(1 << 40, size=s, replace=False).astype(np.uint64)
    db = np.repeat(q[None, :], b + 1, axis=0)
    for i in range(b + 1):
        for j in range(b):
            if j != i:
                t = int(rng.integers(edges[j], edges[j + 1]))
                db[i, t] = q[t] + np.uint64((1 << 41) + i)
    other = (rng.choice(1 << 40, size=(8, s)).astype(np.uint64) + np.uint64(1 << 42))
    return frozen(q[None, :].copy(), np.ascontiguousarray(np.vstack([db, other])))


def check_planted(s, d):
    q, db = planted(s, d)
    u, b = u_max(s, d), default_bands(s, d)
    assert b == u + 1 and ((s, d) != (512, 0.1) or b == 52)
    differ = (db != q).sum(axis=1)
    assert (differ[:b] == u).all() and differ[b] == u + 1
    D = jaccard_blocks(q, db)
    assert (D[0, :b] <= d).all() and D[0, b] > d, NO_TEST + "the planted distances are on the wrong side of the threshold"
    qk, dk = band_keys(q, b), band_keys(db, b)
    same = qk[0][None, :] == dk
    for i in range(b):
        assert same[i].tolist() == [j == i for j in range(b)], NO_TEST + f"band {i} is not the only intact band of sketch {i}"
    assert not same[b:].any(), NO_TEST + "a sketch that differs in every band is a candidate"
    return D, candidates(qk, dk)


# ---- 3. D = 0: exact duplicates among near-copies ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def duplicates(s=33):
    """(queries [3][s], database [200][s]): every database sketch is a copy of a query or differs from it in exactly one slot"""
    rng = np.random.default_rng(8100 + s)
    q = rng.integers(0, 1 << 40, size=(3, s)).astype(np.uint64)
    db = q[rng.integers(0, 3, size=200)].copy()
    for i in range(200):
        if i % 3:
            db[i, int(rng.integers(0, s))] += np.uint64(1 << 41)
    return frozen(q, db)


def check_duplicates(s=33):
    q, db = duplicates(s)
    assert u_max(s, 0.0) == 0 and default_bands(s, 0.0) == 1
    D = jaccard_blocks(q, db)
    assert (D == 0).sum() >= 30 and ((D > 0) & (D < 2 / s)).sum() >= 60, NO_TEST + "copies and near-copies are missing"
    cand = candidates(band_keys(q, 1), band_keys(db, 1))
    assert np.array_equal(cand, D == 0)
    return D, cand


# ---- 4. runs and de-duplication ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def identical(s=33):
    """five queries and 1100 database sketches, all one sketch"""
    one = si.long_inputs(s)[2][:1]
    return frozen(np.repeat(one, si.LONG_M, axis=0), np.repeat(one, si.LONG_P, axis=0))


@functools.lru_cache(maxsize=None)
def copies(s):
    """search_inputs' `copies` database (a run of equal sketches across index 512) under the theorem's threshold"""
    qm = si.long_inputs(s)[0]
    dm, _, D = si.ordered_database(s, "jaccard", "row", "copies")
    d = theorem(s)[3]
    b = default_bands(s, d)
    return qm, dm, D, d, frozen(candidates(band_keys(qm, b), band_keys(dm, b)))[0]


def check_copies(s):
    qm, dm, D, d, cand = copies(s)
    assert not ((D <= d) & ~cand).any()
    run = [int(c) for c in si.COPIES]
    assert len({dm[c].tobytes() for c in run}) == 1
    return cand


# ---- 5. mins as doubles -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def beyond_doubles(s=8):
    """(query [1][s], database [3][s]): sketch 0 differs from the query in every slot as a uint64 and in none as a double (values
    above 2^53), sketch 1 is the query, sketch 2 differs as a double too"""
    q = (np.uint64(1 << 60) + np.arange(s, dtype=np.uint64) * np.uint64(1 << 20))[None, :]
    db = np.vstack([q[0] + np.uint64(1), q[0], q[0] + np.uint64(1 << 12)])
    return frozen(np.ascontiguousarray(q), np.ascontiguousarray(db))


def check_beyond_doubles(s=8):
    q, db = beyond_doubles(s)
    assert (q[0] != db[0]).all() and (q.astype(np.float64)[0] == db.astype(np.float64)[0]).all()
    assert (q.astype(np.float64)[0] != db.astype(np.float64)[2]).all()
    D = jaccard_blocks(q, db)
    assert D[0].tolist() == [0.0, 0.0, 1.0]
    qk, dk = band_keys(q, 1), band_keys(db, 1)
    assert qk[0, 0] == dk[0, 0] == dk[1, 0] != dk[2, 0]
    return D


# ---- 6. fewer bands than the theorem needs ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def few_bands(s=33, bands=2):
    dm, D, d, _, _ = self_case(s)
    keys = band_keys(dm, bands)
    return dm, D, d, bands, frozen(candidates(keys, keys, self_search=True))[0]


def check_few_bands(s=33, bands=2):
    dm, D, d, bands, cand = few_bands(s, bands)
    assert bands < default_bands(s, d)
    off = ~np.eye(len(D), dtype=bool)
    missed = int(((D <= d) & off & ~cand).sum())
    assert missed >= 1, NO_TEST + "every pair within the threshold is a candidate: the filter loses nothing"
    assert ((D <= d) & off & cand).any()
    return missed


# ---- the file format, restated ------------------------------------------------------------------------------------------------------------
MAGIC = b"HULKIDX\n"


def index_file(mins, d, bands, names, version=1):
    """the bytes hulk_index_save writes"""
    mins = np.ascontiguousarray(mins, dtype="<u8")
    n, s = mins.shape
    blob = b"".join(x.encode() + b"\0" for x in names)
    head = MAGIC + struct.pack("<IIII", version, s, n, bands) + struct.pack("<d", d) + struct.pack("<QQ", len(blob), mins.nbytes)
    body = head + blob + mins.tobytes()
    return body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF)
