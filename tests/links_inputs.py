"""The yardstick of tests/test_gpu_links.py and tests/test_links_cpu.py (no test lives here).

From a distance matrix D (oracle.pyorc.smash_matrix, or tests/bottomk_inputs.py's matrix for the bottom-k metric), row i of the links at
tau is np.flatnonzero((D[i] <= tau) & (arange != i)) — ascending j, equality in, a NaN never — and its distances are D[i, those];
the rows one behind the other are CSR.  upper: only j > i.  The inputs are tests/cluster_inputs.py's and tests/bottomk_inputs.py's,
with their own check_* functions; the checks here say what the links tests need of them beyond that."""
import numpy as np

import cluster_inputs as ci

NO_TEST = ci.NO_TEST
METRICS = ("jaccard", "weightedjaccard")


def csr(D, tau, upper=False):
    """-> (indptr uint64[n + 1], indices uint32[E], distances float64[E]) of the definition"""
    n = len(D)
    ar = np.arange(n)
    indptr, indices, distances = [0], [], []
    for i in range(n):
        keep = (D[i] <= tau) & (ar != i)                           # (False for NaN)
        if upper:
            keep &= ar > i
        j = np.flatnonzero(keep)
        indices.append(j.astype(np.uint32)); distances.append(D[i, j].astype(np.float64))
        indptr.append(indptr[-1] + len(j))
    return (np.array(indptr, dtype=np.uint64), np.concatenate(indices) if indices else np.zeros(0, np.uint32),
            np.concatenate(distances) if distances else np.zeros(0, np.float64))


def upper_of(indptr, indices, distances):
    """a CSR result filtered to j > i"""
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr.astype(np.int64)))
    keep = indices > rows
    ptr = np.zeros(n + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum(np.bincount(rows[keep], minlength=n))
    return ptr, indices[keep], distances[keep]


def assert_same(got, want, what):
    """indptr, indices and the distance BITS"""
    gp, gi, gd = got
    wp, wi, wd = want
    assert gp.dtype == np.uint64 and gi.dtype == np.uint32 and gd.dtype == np.float64, (what, gp.dtype, gi.dtype, gd.dtype)
    assert gp.shape == wp.shape and np.array_equal(gp, wp), f"{what}: indptr differs, first at row {np.flatnonzero(gp != wp)[:3].tolist() if gp.shape == wp.shape else (gp.shape, wp.shape)}"
    assert np.array_equal(gi, wi), f"{what}: indices differ, first at edge {np.flatnonzero(gi != wi)[:3].tolist()}"
    gb, wb = gd.view(np.uint64), wd.view(np.uint64)
    assert np.array_equal(gb, wb), f"{what}: distance bits differ, first at edge {np.flatnonzero(gb != wb)[:3].tolist()}"


def degrees(indptr):
    return np.diff(indptr.astype(np.int64))


def check_chain_links(s):
    """the planted chains at their tau: exactly the chain-neighbour links, both directions, among them pairs across the tile edges
    of the subjects (32) and the others (64) and across the band edges of band_rows 32 and 96; one ulp below, none"""
    mins, weights, D, members = ci.planted_chains(s)
    tau, _ = ci.check_planted_chains(s)
    ptr, idx, dist = csr(D["jaccard"], tau)
    want = sorted((a, b) for m in members for x, y in zip(m, m[1:]) for a, b in ((x, y), (y, x)))
    rows = np.repeat(np.arange(257), degrees(ptr))
    assert sorted(zip(rows.tolist(), idx.tolist())) == want, NO_TEST + "the links are not the chain neighbours"
    assert (dist == tau).all(), NO_TEST + "a link that is not exactly at tau"
    for a, b in ci.BRIDGES:
        assert (a, b) in want and (b, a) in want, NO_TEST + f"{(a, b)} is no link"
    assert int(csr(D["jaccard"], np.nextafter(tau, 0.0))[0][-1]) == 0, NO_TEST + "one ulp below tau something still links"
    return tau


def check_weighted_links():
    """what the weighted set shows of a DIRECTED list"""
    mins, weights, D = ci.weighted_set()
    ci.check_weighted_set()
    out = {t: csr(D, t) for t in (0.0, 0.5, 1.0)}
    ptr, idx, _ = out[0.5]

    def row(i):
        return idx[int(ptr[i]):int(ptr[i + 1])].tolist()
    assert ci.X1 in row(ci.X0) and ci.X0 not in row(ci.X1), NO_TEST + "(X0, X1) is not a one-direction link"
    assert row(ci.Z) == [] and ci.Z in row(ci.Y), NO_TEST + "the NaN subject"
    for t in out:
        p, i, _ = out[t]
        assert int(p[ci.Z + 1] - p[ci.Z]) == 0, NO_TEST + "the NaN subject has links"
    p, i, d = out[1.0]
    u = i[int(p[ci.U]):int(p[ci.U + 1])].tolist()
    assert ci.V not in u and ci.I0 in u, NO_TEST + "the Inf weight: NaN against V, 1.0 against the others"
    p, i, d = out[0.0]
    assert ci.I1 in i[int(p[ci.I0]):int(p[ci.I0 + 1])].tolist() and ci.I0 in i[int(p[ci.I1]):int(p[ci.I1 + 1])].tolist(), NO_TEST + "the identical pair at tau 0"
    assert int(p[-1]) > 0
    return out


def check_random_links(s):
    """at tau = 1.0 every non-NaN off-diagonal pair is listed: rows span all five column tiles, jaccard's largest degree is 256"""
    mins, weights, per_metric = ci.random_set(s)
    ci.check_random_set(s)
    for metric in METRICS:
        D, taus = per_metric[metric]
        ptr, idx, _ = csr(D, 1.0)
        off = ~np.eye(257, dtype=bool)
        assert int(ptr[-1]) == int((~np.isnan(D) & off).sum()), NO_TEST + "tau = 1 does not list every non-NaN pair"
        if metric == "jaccard":
            assert degrees(ptr).max() == 256 and degrees(ptr).min() == 256, NO_TEST + "jaccard at tau = 1: every row is full"
        tiles = {int(j) // 64 for j in idx[int(ptr[100]):int(ptr[101])]}
        assert tiles == {0, 1, 2, 3, 4}, NO_TEST + "a row that does not span the five column tiles"


def render_csv(order, got):
    """the file hulk_links_files writes, from a CSR result over the sorted paths `order`"""
    from hulk_amd.smash import go_csv_field, go_format_f2
    ptr, idx, dist = got
    lines = ["sketch,neighbour,distance,similarity\n"]
    for i in range(len(order)):
        for e in range(int(ptr[i]), int(ptr[i + 1])):
            d = float(dist[e])
            lines.append(f"{go_csv_field(order[i])},{go_csv_field(order[int(idx[e])])},{'%.17g' % d},{go_format_f2(100 - (d * 100))}\n")
    return "".join(lines)
