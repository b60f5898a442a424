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


# ---- 7. the staging buffer's second piece ---------------------------------------------------------------------------------------------------
# upload_rows (hulk_index.hip) sends raw mins up INDEX_STAGE = 2^23 entries at a time; piece k lands at d_out + k * 2^23.  At S = 512
# the first piece is 16,384 sketches exactly, and 64 more make a second one — on the build side for the database and on the query
# side for as many queries.  The arrays are 67 MB each and are NOT cached: the tests free them when they are done.
STAGE_S, STAGE_N, STAGE_D = 512, 16448, 0.05
STAGE_BORDER = (1 << 23) // STAGE_S                                # 16,384: the first sketch of the second piece
STAGE_COPIES = (0, 1, STAGE_BORDER - 1, STAGE_BORDER, STAGE_N - 1)  # rows with a byte-identical query
STAGE_NEAR = tuple(range(STAGE_BORDER - 4, STAGE_BORDER + 4))      # rows with a query that differs in u_max slots: a hit at the threshold's edge
STAGE_FAR = tuple(range(STAGE_BORDER - 8, STAGE_BORDER - 4)) + tuple(range(STAGE_BORDER + 4, STAGE_BORDER + 8))    # ... in u_max + 1 slots: none
STAGE_K = 2


def stage_constants():
    import os
    import re
    text = open(os.path.join(si.ROOT, "hulk_amd", "csrc", "hulk_index.hip")).read()
    m = re.search(r"constexpr size_t INDEX_STAGE = (\d+)u << (\d+);", text)
    return int(m.group(1)) << int(m.group(2))


def stage_database():
    """[16448][512] random 50-bit mins (any two rows differ in every slot: check_stage_database)"""
    return np.random.default_rng(8200).integers(0, 1 << 50, size=(STAGE_N, STAGE_S), dtype=np.uint64)


def stage_near_copy(rng, row, differ, spread):
    """row with `differ` slots replaced by values no row holds (above 2^50); spread: one in each of the first `differ` bands"""
    out = row.copy()
    if spread:
        edges = band_edges(STAGE_S, default_bands(STAGE_S, STAGE_D))
        at = [int(rng.integers(edges[j], edges[j + 1])) for j in range(differ)]
    else:
        at = rng.choice(STAGE_S, size=differ, replace=False)
    out[at] = (np.uint64(1 << 51) + rng.integers(0, 1 << 40, size=differ, dtype=np.uint64))
    return out


def stage_query(rng, db, r, kind):
    """the query made of database row r -> (query, its distance from r as the kernels compute it, or None if r is no hit)"""
    u = u_max(STAGE_S, STAGE_D)
    if kind == "near":
        return stage_near_copy(rng, db[r], u, spread=False), 1.0 - (float(STAGE_S - u) / float(STAGE_S))
    if kind == "far":
        return stage_near_copy(rng, db[r], u + 1, spread=(r % 2 == 0)), None
    return db[r].copy(), 0.0


def stage_build_queries(db):
    """64 queries with their hits in both pieces of the database -> (queries [64][512], [(the row a query was made of, its kind)])"""
    rng = np.random.default_rng(8201)
    plan = [(r, "copy") for r in STAGE_COPIES] + [(r, "near") for r in STAGE_NEAR] + [(r, "far") for r in STAGE_FAR]
    rest = [r for r in rng.permutation(STAGE_N).tolist() if r not in STAGE_COPIES + STAGE_NEAR + STAGE_FAR]
    plan += [(r, "copy") for r in [r for r in rest if r < STAGE_BORDER][:22] + [r for r in rest if r >= STAGE_BORDER][:21]]
    plan = [plan[i] for i in rng.permutation(len(plan)).tolist()]
    return np.array([stage_query(rng, db, r, kind)[0] for r, kind in plan], dtype=np.uint64), plan


def stage_distances(qm, db):
    """[m][n] jaccard distances in numpy: 1.0 - (slots equal as doubles) / S, the yardstick's expression (mins below 2^53 are exact)"""
    out = np.empty((len(qm), len(db)))
    for i, q in enumerate(qm):
        out[i] = 1.0 - ((db == q).sum(axis=1).astype(np.float64) / float(STAGE_S))
    return out


def stage_candidates(qm, db, D):
    """[m][n] bool from band_keys — computed for the database rows that share a slot with some query; a row that shares none has no
    band in common with any query and equal keys would be a collision of the 64-bit hash"""
    b = default_bands(STAGE_S, STAGE_D)
    related = np.flatnonzero((D < 1.0).any(axis=0))
    cand = np.zeros(D.shape, dtype=bool)
    cand[:, related] = candidates(band_keys(qm, b), band_keys(db[related], b))
    return cand, related


def check_stage_database(db):
    assert stage_constants() == 1 << 23 and STAGE_BORDER * STAGE_S == 1 << 23 < STAGE_N * STAGE_S, NO_TEST + "the database fits one piece"
    assert (STAGE_N - STAGE_BORDER) * STAGE_S < 1 << 23 and u_max(STAGE_S, STAGE_D) == 25 and default_bands(STAGE_S, STAGE_D) == 26
    rng = np.random.default_rng(8202)
    for a, b in rng.integers(0, STAGE_N, size=(200, 2)).tolist():
        assert a == b or not (db[a] == db[b]).any(), NO_TEST + f"rows {a} and {b} share a slot"
    for r in STAGE_COPIES + STAGE_NEAR + STAGE_FAR:
        assert np.flatnonzero((db == db[r]).any(axis=1)).tolist() == [r], NO_TEST + f"row {r} shares a slot with another row"


def check_stage_build(db, qm, plan):
    """-> (D [64][n], candidates): every query is at 1.0 from every row but its own; copies at 0, near-copies at the last distance
    within the threshold, the others one slot beyond it; hits on both sides of the border"""
    u, d = u_max(STAGE_S, STAGE_D), STAGE_D
    D = stage_distances(qm, db)
    cand, related = stage_candidates(qm, db, D)
    rows = [r for r, _ in plan]
    assert sorted(related.tolist()) == sorted(set(rows)) and len(plan) == 64, NO_TEST + "a query is related to another row than its own"
    for i, (r, kind) in enumerate(plan):
        assert np.flatnonzero(D[i] < 1.0).tolist() == [r]
        differ = int((qm[i] != db[r]).sum())
        assert differ == {"copy": 0, "near": u, "far": u + 1}[kind], NO_TEST + f"query {i} of row {r} differs in {differ} slots"
        assert (D[i, r] <= d) == (kind != "far") and (kind == "far" or cand[i, r]), NO_TEST + f"query {i} of row {r}"
        if kind == "far":
            assert cand[i, r] == (r % 2 == 1), NO_TEST + "a far copy with a slot in every band is no candidate, one with an intact band is"
    assert int(cand.sum()) == 64 - len(STAGE_FAR) // 2
    hit = np.array([r for i, (r, kind) in enumerate(plan) if kind != "far"])
    assert (hit < STAGE_BORDER).sum() >= 20 and (hit >= STAGE_BORDER).sum() >= 20, NO_TEST + "too few hits on one side of the border"
    for r in STAGE_COPIES:
        assert (r, "copy") in plan
    sub = np.array(sorted(set(rows) | set(range(60, 70))))
    assert np.array_equal(bits_of(D[:, sub]), bits_of(jaccard_blocks(qm, db[sub]))), "the numpy distances are not the oracle's"
    return D, cand


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def stage_full_queries(db):
    """16,448 queries, query i made of row perm[i]: a copy, but for the queries on either side of the border of the QUERY side
    (STAGE_NEAR: u_max slots differ, STAGE_FAR: u_max + 1) -> (queries, perm, the expected (index [m][2], distance, count))"""
    rng = np.random.default_rng(8203)
    perm = rng.permutation(STAGE_N)
    u = u_max(STAGE_S, STAGE_D)
    qm = db[perm]                                                    # (a copy)
    index = np.full((STAGE_N, STAGE_K), NONE, dtype=np.uint32); dist = np.full((STAGE_N, STAGE_K), np.nan); count = np.ones(STAGE_N, dtype=np.uint32)
    index[:, 0] = perm; dist[:, 0] = 0.0
    for i in STAGE_NEAR:
        qm[i] = stage_near_copy(rng, db[perm[i]], u, spread=False)
        dist[i, 0] = 1.0 - (float(STAGE_S - u) / float(STAGE_S))
    for i in STAGE_FAR:
        qm[i] = stage_near_copy(rng, db[perm[i]], u + 1, spread=(i % 2 == 0))
        index[i, 0] = NONE; dist[i, 0] = np.nan; count[i] = 0
    return qm, perm, (index, dist, count)


def check_stage_full(db, qm, perm, want):
    index, dist, count = want
    assert sorted(perm.tolist()) == list(range(STAGE_N)), NO_TEST + "not a permutation"
    assert (perm[:STAGE_BORDER] >= STAGE_BORDER).any() and (perm[STAGE_BORDER:] < STAGE_BORDER).any()
    differ = (qm != db[perm]).sum(axis=1)
    u = u_max(STAGE_S, STAGE_D)
    assert sorted(np.flatnonzero(differ).tolist()) == sorted(STAGE_NEAR + STAGE_FAR), NO_TEST + "the planted queries are not around the border"
    assert (differ[list(STAGE_NEAR)] == u).all() and (differ[list(STAGE_FAR)] == u + 1).all()
    assert (count[list(STAGE_FAR)] == 0).all() and int(count.sum()) == STAGE_N - len(STAGE_FAR)
    assert (dist[list(STAGE_NEAR), 0] <= STAGE_D).all() and (dist[list(STAGE_NEAR), 0] > 0).all()
    # by construction a query shares slots with its own row alone; held to the oracle on the planted queries and a sample
    rng = np.random.default_rng(8204)
    some = np.array(sorted(set(STAGE_NEAR + STAGE_FAR + STAGE_COPIES) | set(rng.integers(0, STAGE_N, size=20).tolist())))
    D = stage_distances(qm[some], db)
    got = select(D, STAGE_K, max_distance=STAGE_D)
    for g, w in zip(got, (index[some], dist[some], count[some])):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), NO_TEST + "the expected lists are not the yardstick's"
    assert ((D < 1.0).sum(axis=1) == 1).all(), NO_TEST + "a query shares a slot with another row than its own"


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
