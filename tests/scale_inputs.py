"""The inputs, yardsticks and check_* functions of tests/test_gpu_collection_scale.py and tests/test_collection_scale_cpu.py (no
test lives here): hulk_cluster, hulk_dendrogram and hulk_links past the sizes their own suites run at.

N = 4161 = 65 * 64 + 1: NP = 4224, 66 column tiles (the last holds one column) and 131 row tiles — about 4.4 k workgroups a launch
for the symmetric metrics and 8,646 for weighted jaccard, many times what a device holds at once, and the first size at which
k_dendro_fold's strided loops (`c += 64` over the column tiles of a row, `r += 64` over the row tiles of a band) take a second trip.
S = 8 throughout (the tile's slot loop is tested elsewhere): the oracle stays cheap and jaccard ties everywhere.

Yardstick: oracle.pyorc.smash_matrix over the whole set for jaccard and weighted jaccard; for bottomk the GPU's own matrix, held
to bottomk_inputs.matrix on a 64-sketch sample (the GPU tests do that before they use it).  Everything else goes from the matrix
through the restatements the suite has: cluster_inputs.components, dendrogram_inputs.kruskal / cut_labels, links_inputs.csr.

The sets are cluster_inputs.chain plus fresh random sketches, mins below 2^50.  Any two sketches that are not within three chain
steps of each other share no slot and are at 1.0 under every metric: 99.86 % of the pairs.  The 1 % and 10 % quantiles of ALL
off-diagonal distances are therefore 1.0, where everything is one cluster; the thresholds used are those quantiles of the distances
BELOW 1.0 (method "lower": a distance that occurs), the ones at which `1 < clusters < N` can hold."""
import functools

import numpy as np

import cluster_inputs as ci
import dendrogram_inputs as di
from oracle import pyorc

NO_TEST = ci.NO_TEST
N, S = 4161, 8
T0 = ci.T0[S]
TAU = ci.chain_tau(S)
METRICS = ("jaccard", "weightedjaccard", "bottomk")
ORACLE_METRICS = ("jaccard", "weightedjaccard")
CHAIN_SIZES = (2100, 1100, 500, 300, 100)                           # the other 61 sketches are singletons
CLUSTER_BANDS = (0, 32, 4192)                                       # three bands (no flatten between them), 131 bands, one band
DENDRO_BANDS = (0, 2080, 4192)                                      # 2080: 65 row tiles in the first band, 4192: 131 in the only one
LINKS_BANDS = (0, 4192)
ORDERS = ("ascending", "descending", "random")
ROUNDS_CASE = ("chains", "jaccard")                                 # the case whose number of rounds is held to the offer form
SAMPLE = 64                                                         # sketches of the bottomk anchor

# far_pairs: three groups of two HUBS (byte-identical twins, the smaller index first) and eight WITNESSES; witness k is the hub with
# slot k fresh.  A witness is at 1/8 from both hubs and at 2/8 from the other witnesses of its group; the hubs are at 0 from each
# other.  So a witness's nearest partner is the first hub, the hub's own nearest is its twin (never the witness), the witness's
# runner-up is the second hub, and {witness, second hub} closes the cycle witness - hub - twin: no edge of the forest.
#   ROW   hubs in column tiles 64 and 65, witnesses in front of row 2048: the witness's row minimum over column tile 64 is the
#         65th entry of its row of partials — the second trip of `for (c = qt0 + lane; c < CT; c += 64)`
#   COL2  hubs in row tile 64 of the first band (band_rows 2080 and 4192), witnesses behind them: the witness's column minimum
#         from that row tile is the 65th entry of its row of column partials — the second trip of `for (r = lane; r < rt; r += 64)`
#   COL3  hubs in row tile 129 of the only band at band_rows 4192 (the third trip) and in row tile 64 of the second band at 2080
# Weighted jaccard takes both weight vectors from the subject: d(s, q) is the share of s's weight on the slots where they differ.
# The hubs weigh 1 everywhere (1/8 towards a witness).  A ROW witness weighs 2^-20 on its fresh slot — its own row holds the
# smaller direction; a COL witness weighs 64 there — the hub's row holds the smaller direction and the witness receives it as a column.
GROUPS = {"ROW": ((4097, 4160), (3, 31, 40, 100, 700, 1500, 2000, 2047)),
          "COL2": ((2050, 2070), (2060, 2100, 2500, 3000, 3500, 4000, 4095, 4120)),
          "COL3": ((4130, 4131), (4132, 4133, 4134, 4135, 4136, 4137, 4138, 4139))}
WITNESS_WEIGHT = {"ROW": 2.0 ** -20, "COL2": 64.0, "COL3": 64.0}
RESERVED = tuple(sorted(i for hubs, wit in GROUPS.values() for i in hubs + wit))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def band_of(band_rows):
    return band_rows or 2048                                        # (the default of hulk_cluster, hulk_dendrogram and hulk_links)


def band_start(i, band_rows):
    return i // band_of(band_rows) * band_of(band_rows)


# ---- the sets --------------------------------------------------------------------------------------------------------------------
def build_set(seed, reserved=()):
    """five chains (CHAIN_SIZES) and fresh random sketches on the indices outside `reserved`, placed by a fixed permutation; the
    reserved indices hold fresh random sketches until far_pairs overwrites them.  -> (mins, weights, members)"""
    rng = np.random.default_rng(seed)
    taken = set(reserved)
    free = [i for i in rng.permutation(N).tolist() if i not in taken]
    mins = rng.integers(0, 1 << 50, size=(N, S), dtype=np.uint64)
    members = []
    for size in CHAIN_SIZES:
        idx = [free.pop() for _ in range(size)]
        mins[idx] = ci.chain(rng, size, S, T0)
        members.append(idx)
    weights = -rng.gamma(2.0, 1e-3, size=(N, S))
    return mins, weights, members


def matrices(mins, weights):
    return {m: pyorc.smash_matrix(mins, weights, m) for m in ORACLE_METRICS}


@functools.lru_cache(maxsize=None)
def chains():
    """-> (mins, weights, {metric: D}, members): ties everywhere under jaccard, several Boruvka rounds"""
    mins, weights, members = build_set(9100)
    D = matrices(mins, weights)
    frozen(mins, weights, *D.values())
    return mins, weights, D, members


@functools.lru_cache(maxsize=None)
def far_pairs():
    """chains' construction with the 30 sketches of GROUPS planted among the singletons -> (mins, weights, {metric: D}, members)"""
    mins, weights, members = build_set(9200, RESERVED)
    rng = np.random.default_rng(9201)
    for name, (hubs, wit) in GROUPS.items():
        hub = rng.integers(0, 1 << 50, size=S, dtype=np.uint64)
        for h in hubs:
            mins[h] = hub; weights[h] = -1.0
        for k, w in enumerate(wit):
            mins[w] = hub
            mins[w, k] = rng.integers(0, 1 << 50, dtype=np.uint64)
            weights[w] = -1.0
            weights[w, k] = -WITNESS_WEIGHT[name]
    D = matrices(mins, weights)
    frozen(mins, weights, *D.values())
    return mins, weights, D, members


@functools.lru_cache(maxsize=None)
def one_chain(order):
    """cluster_inputs.ordered_chain's three orders at this N and S: at chain_tau(8) every link is a bridge -> (mins, weights, D)"""
    rng = np.random.default_rng(9300)
    c = ci.chain(rng, N, S, T0)
    place = {"ascending": np.arange(N), "descending": np.arange(N)[::-1], "random": np.random.default_rng(9301).permutation(N)}[order]
    mins = np.empty_like(c)
    mins[place] = c
    weights = -rng.gamma(2.0, 1e-3, size=(N, S))
    return frozen(mins, weights, pyorc.smash_matrix(mins, weights, "jaccard"))


SETS = {"chains": chains, "far_pairs": far_pairs}


def sample_rows(name):
    """the 64 sketches of the bottomk anchor: 34 at random and, for far_pairs, every planted sketch"""
    rng = np.random.default_rng(9400)
    fixed = list(RESERVED) if name == "far_pairs" else []
    rest = [i for i in rng.permutation(N).tolist() if i not in set(fixed)]
    return np.sort(np.array(fixed + rest[:SAMPLE - len(fixed)]))


# ---- the yardsticks, cached per (set, metric); D_bottomk is the anchored GPU matrix of the caller ---------------------------------------
_given = {}


def give_matrix(name, metric, D):
    """the GPU tests hand over the anchored bottomk matrix of a set here (once per process; read-only from then on)"""
    if (name, metric) not in _given:
        D = np.array(D, dtype=np.float64)
        D.setflags(write=False)
        _given[(name, metric)] = D
    return _given[(name, metric)]


def matrix(name, metric):
    if metric in ORACLE_METRICS:
        return SETS[name]()[2][metric]
    assert (name, metric) in _given, "the bottomk matrix comes from the GPU: give_matrix() first"
    return _given[(name, metric)]


@functools.lru_cache(maxsize=None)
def forest(name, metric):
    return frozen(*di.kruskal(matrix(name, metric)))


@functools.lru_cache(maxsize=None)
def thresholds(name, metric):
    """chain_tau(8) and the 1 % and 10 % quantiles of the off-diagonal distances below 1.0 (the module's docstring), without repeats"""
    D = matrix(name, metric)
    off = D[~np.eye(N, dtype=bool)]
    near = off[off < 1.0]                                           # (False for NaN)
    out = [TAU]
    for q in (0.01, 0.10):
        t = float(np.quantile(near, q, method="lower"))
        if t not in out:
            out.append(t)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def clustering(name, metric, tau):
    labels, links, clusters = ci.components(matrix(name, metric), tau)
    labels.setflags(write=False)
    return labels, links, clusters


@functools.lru_cache(maxsize=None)
def chain_clustering(order, below):
    D = one_chain(order)[2]
    labels, links, clusters = ci.components(D, float(np.nextafter(TAU, 0.0)) if below else TAU)
    labels.setflags(write=False)
    return labels, links, clusters


# ---- the checks -------------------------------------------------------------------------------------------------------------------
def first_round(D):
    """round 1 of the offer form (comp = the identity): per sketch (p, runner-up) by the lexicographic order (W bits, partner)"""
    W = di.edge_weights(np.asarray(D, dtype=np.float64))
    key = np.where(np.isnan(W), np.inf, W)                          # (W >= 0: the order of the bits is the order of the doubles)
    p = key.argmin(axis=1)                                          # the first minimum: the smaller partner at equal W
    key[np.arange(len(key)), p] = np.inf
    return W, p, key.argmin(axis=1)


def check_far_pairs(metric):
    """the second (and third) trip of k_dendro_fold's two loops decides at least 8 sketches each, and losing it shows: the issue's
    witness conditions on round 1, for every band_rows the dendrogram tests use.  -> {path: witnesses}"""
    D = matrix("far_pairs", metric)
    W, p, second = first_round(D)
    a, b, _ = forest("far_pairs", metric)
    in_forest = set(zip(a.tolist(), b.tolist()))
    weighted = metric == "weightedjaccard"

    def sound(i):                                                   # the other end does not offer the same edge; the runner-up is no forest edge
        return p[p[i]] != i and (min(i, int(second[i])), max(i, int(second[i]))) not in in_forest and not np.isnan(W[i, p[i]])

    out = {}
    for band in DENDRO_BANDS:
        rows = []
        for i in range(N):
            pi = int(p[i])
            if weighted:
                hit = D[i, pi] < D[pi, i] and pi >= 4096
            else:
                hit = pi > i and pi // 64 - band_start(i, band) // 64 >= 64
            if hit and sound(i):
                rows.append(i)
        assert len(rows) >= 8, NO_TEST + f"{metric} band_rows {band}: {len(rows)} sketches need the second trip of the row loop"
        out[("row", band)] = rows
        if band_of(band) <= 2048:
            continue                                                # (at most 64 row tiles a band: the column loop takes one trip)
        cols = {64: [], 128: []}
        for q in range(N):
            s = int(p[q])
            if not ((D[s, q] < D[q, s]) if weighted else s < q) or not sound(q):
                continue
            tile = (s - band_start(s, band)) // 32
            for least in cols:
                if tile >= least:
                    cols[least].append(q)
        assert len(cols[64]) >= 8, NO_TEST + f"{metric} band_rows {band}: {len(cols[64])} sketches need the second trip of the column loop"
        if band == 4192:
            assert len(cols[128]) >= 2, NO_TEST + f"{metric}: {len(cols[128])} sketches need the third trip of the column loop"
        out[("col", band)] = cols[64]
        out[("col3", band)] = cols[128]
    # the planted sketches are what they were planted as
    for name, (hubs, wit) in GROUPS.items():
        assert W[hubs[0], hubs[1]] == 0, NO_TEST + f"{name}: the hubs are no twins"
        for w in wit:
            assert int(p[w]) == hubs[0] and int(second[w]) == hubs[1] and W[w, hubs[0]] == W[w, hubs[1]] < 0.25, NO_TEST + f"{name}: witness {w}"
            assert w in (out[("row", 0)] if name == "ROW" else out[("col", 4192)]), NO_TEST + f"{name}: witness {w} is not counted"
            if name == "COL3":
                assert w in out[("col3", 4192)] and w in out[("col", 2080)], NO_TEST + f"COL3: witness {w}"
            if name == "COL2":
                assert w in out[("col", 2080)], NO_TEST + f"COL2: witness {w}"
    return out


def check_chains(name, metric):
    """at every threshold used something links and not everything does; weighted jaccard's tree has at least 3 distinct heights,
    the symmetric metrics' trees have tied ones"""
    out = {}
    for tau in thresholds(name, metric):
        labels, links, clusters = clustering(name, metric, tau)
        assert 0 < links and 1 < clusters < N, NO_TEST + f"{name} {metric} tau {tau!r}: {links} links, {clusters} clusters"
        out[tau] = (links, clusters)
    heights = len(np.unique(forest(name, metric)[2]))
    if metric == "weightedjaccard":
        assert heights >= 3, NO_TEST + f"{name}: {heights} heights"
    else:
        assert heights < len(forest(name, metric)[2]), NO_TEST + f"{name} {metric}: no tied heights"
        labels = clustering(name, metric, TAU)[0]
        for idx in SETS[name]()[3]:
            assert (labels[idx] == min(idx)).all(), NO_TEST + "a chain is not one component at its tau"
    return out


@functools.lru_cache(maxsize=None)
def rounds(name, metric):
    """the passes of the offer form (dendrogram_inputs.offer_rounds), which must reproduce Kruskal"""
    a, b, d, r = di.offer_rounds(matrix(name, metric))
    assert di.same_edges((a, b, d), forest(name, metric)), NO_TEST + "the offer form does not reproduce Kruskal"
    assert 4 <= r <= di.round_bound(N), NO_TEST + f"{r} rounds"
    return r


def check_one_chain(order):
    labels, links, clusters = chain_clustering(order, False)
    assert clusters == 1 and not labels.any() and links == 2 * (N - 1), NO_TEST + "the chain is not one component held by neighbour links"
    assert chain_clustering(order, True)[2] == N, NO_TEST + "one ulp below tau something still links"
    return labels, links, clusters
