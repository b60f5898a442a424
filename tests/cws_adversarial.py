"""Adversarial inputs for the CWS resolve (hulk_cws.hip): seeded generators that put the flush at the edges its logic has —
near-ties below fp32 resolution, exact fp64 ties, more than 64 tied wave tiles, elements at the weight's margin — plus what
certifies them: a 50-digit evaluation of getSample (mpmath) and a one-slot replay of AddElement in numpy.

Shared by tests/test_cws_adversarial_cpu.py (generators, certificates, oracle against replay: no GPU) and
tests/test_gpu_cws_adversarial.py (the same seeded scenarios on the device).  No test lives here.

How a scenario is built: the count-min estimate `f` of every AddElement call does not depend on the CWS tables, so the oracle
is run once with tracing on (pyorc.Sketcher.trace), and the tables are chosen afterwards, knowing every f.

Gaps and what they rest on.  getSample is  A = c / (exp(log f - b) * exp(r)).  With exp and log correct to ~1 ulp, its relative
error in fp64 is below (|log f| + |b| + |r| + 4) * 2^-52 < 1e-14 for arguments under 40, on glibc and on the device alike.  A planted
near-tie has a relative gap of at least 1e-12 (certified at 50 digits from the ROUNDED table entries): a factor 100 above that
error, so both libms must order the pair the same way.  Exact ties are made from IDENTICAL inputs (same r, c, b, f), which give
identical outputs on either side; classes of distinct inputs are certified to be at least 1e-9 apart.
With concept drift the device's count-min is a re-association of the reference's step-by-step scaling (hulk_countmin.hip:
~1e-13 relative in f, hence in A), so the gaps planted there start at 1e-10: a factor 1000.
"""
import functools
import math

import numpy as np

from oracle import pyorc

K, W = 15, 9
B = K ** 4                      # 50625 bins
TILE = 256                      # bins per wave tile of the scan (SCAN_TILE / 4)
NTILES = (B + TILE - 1) // TILE  # 198, the last one holds 193 bins
MAXF = np.finfo(np.float64).max
# both signs of every gap are planted; 2e-5 lies outside the 1e-5 band of the fp32 screen
DELTAS = (1e-12, 1e-10, 1e-9, 3e-8, 2e-7, 1e-6, 9e-6)
DELTA_OUT = 2e-5
DRIFT_DELTAS = (1e-10, 1e-9, 3e-8, 2e-7, 1e-6, 9e-6, 2e-5)
MIN_GAP = 1e-12


def mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


# ---- the formula ------------------------------------------------------------------------------------------------------------
def A64(r, c, b, f):
    """CWS.getSample (histosketch.go:30-33), literal, fp64."""
    return c / (np.exp(np.log(f) - b) * np.exp(r))


def A_mp(r, c, b, f):
    """... at 50 digits, from the fp64 values as they stand in the table."""
    m = mp()
    r, c, b, f = (m.mpf(float(v)) for v in (r, c, b, f))
    return c / (m.exp(m.log(f) - b) * m.exp(r))


def solve_c(target, r, b, f):
    """the fp64 c nearest to the one that gives getSample == target (an mpf)"""
    m = mp()
    r, b, f = (m.mpf(float(v)) for v in (r, b, f))
    return float(target * m.exp(m.log(f) - b) * m.exp(r))


def plant_relative(tab, s, y, fy, ref, delta):
    """Set c[s, y] so that A_y = ref * (1 + delta) (ref: mpf, not 0), then move it ulp by ulp until the realised gap is not
    below the designed one.  Returns the realised relative gap A_y / ref - 1 as a float."""
    r, c, b = tab
    want = ref * (1 + mp().mpf(delta))
    c[s, y] = solve_c(want, r[s, y], b[s, y], fy)
    for _ in range(8):
        gap = A_mp(r[s, y], c[s, y], b[s, y], fy) / ref - 1
        if abs(gap) >= abs(delta):
            break
        c[s, y] = np.nextafter(c[s, y], c[s, y] * 2 if delta > 0 else 0.0)
    return float(A_mp(r[s, y], c[s, y], b[s, y], fy) / ref - 1)


def gap_ok(gap, delta):
    """the certificate of a planted gap: within 1 % of the design and at least MIN_GAP"""
    return abs(gap / delta - 1) < 0.01 and abs(gap) >= MIN_GAP and (gap > 0) == (delta > 0)


def base_tables(rng, S):
    """tables as newCWS draws them: r ~ Gamma(2,1), c = ln Gamma(2,1), b = U * r"""
    r = rng.gamma(2.0, 1.0, size=(S, B))
    c = np.log(rng.gamma(2.0, 1.0, size=(S, B)))
    b = rng.random((S, B)) * r
    return r, c, b


# ---- the stream ---------------------------------------------------------------------------------------------------------------
class Scenario:
    """One input: S slots, tables, a stream (spectra for add_histogram + flush, or reads under the interval rule), and what
    the generator designed: `winners` {(flush, slot): bin expected in `mins` after that flush}, `gaps` [(designed, realised)]."""
    def __init__(self, name, S, tables, decay=1.0, spectra=None, reads=None, interval=0, n_int=0):
        self.name, self.S, self.tables, self.decay = name, S, tables, decay
        self.spectra, self.reads, self.interval, self.n_int = spectra, reads, interval, n_int
        self.winners, self.gaps, self.info = {}, [], {}
        self.trace = None

    @property
    def n_flush(self):
        return len(self.spectra) if self.spectra is not None else self.n_int

    def piece(self, t):
        bases, offsets = self.reads
        L = int(offsets[1])
        I = self.interval
        return bases[t * I * L:(t + 1) * I * L], np.arange(I + 1, dtype=np.uint64) * np.uint64(L)


def _feed(o, spectra, reads, interval, n_int, each):
    if spectra is not None:
        for h in spectra:
            o.add_histogram(h); o.flush(); each(o)
    else:
        bases, offsets = reads
        L = int(offsets[1])
        for t in range(n_int):
            o.add_reads(bases[t * interval * L:(t + 1) * interval * L], np.arange(interval + 1, dtype=np.uint64) * np.uint64(L))
            each(o)


def stream_trace(decay=1.0, spectra=None, reads=None, interval=0, n_int=0):
    """[(bins int64[n_t], f float64[n_t]) per flush]: the AddElement stream of the oracle (one slot: f needs no tables)"""
    o = pyorc.Sketcher(K, W, 1, B, decay, interval)
    o.trace()
    _feed(o, spectra, reads, interval, n_int, lambda _o: None)
    fl, bn, f = o.get_trace()
    o.close()
    n = len(spectra) if spectra is not None else n_int
    assert fl.max() == n - 1
    return [(bn[fl == t].astype(np.int64), f[fl == t]) for t in range(n)]


def oracle_states(sc):
    """(mins uint64[n_flush][S], weights float64[n_flush][S]): the oracle's sketch after every flush"""
    o = pyorc.Sketcher(K, W, sc.S, B, sc.decay, sc.interval)
    o.set_cws_tables(*sc.tables)
    ms, ws = [], []

    def each(o_):
        m, w = o_.sketch(); ms.append(m); ws.append(w)
    _feed(o, sc.spectra, sc.reads, sc.interval, sc.n_int, each)
    if sc.reads is not None:                                    # (whole intervals: the final flush finds nothing left)
        o.finish()
        m, w = o.sketch()
        assert np.array_equal(m, ms[-1]) and np.array_equal(w, ws[-1])
    o.close()
    return np.stack(ms), np.stack(ws)


def replay_slot(trace, r_row, c_row, b_row, decay_weight=None, upto=None, strict=True):
    """AddElement's update rule for ONE slot in stream order, A by the literal formula in fp64 (numpy):
    no drift (decay_weight None): if A < w;  drift: if A < w / decay_weight  (histosketch.go:139-153).
    Returns [(min, weight) after every flush].  upto = (flush, position): stop in front of that element and return (min, weight).
    strict=False: the drift rule with <= (a wrong rule, to show that a case tells the two apart)."""
    w, m = MAXF, 0
    out = []
    for t, (bins, f) in enumerate(trace):
        n = len(bins)
        if upto is not None and upto[0] == t:
            n = upto[1]
        A = A64(r_row[bins[:n]], c_row[bins[:n]], b_row[bins[:n]], f[:n])
        if decay_weight is None:
            if n:
                i = int(np.argmin(A))                   # the first of equal minima: the earliest element
                if A[i] < w:
                    w, m = float(A[i]), int(bins[i])
        else:
            pos = 0
            while pos < n:
                with np.errstate(over="ignore"):
                    th = np.float64(w) / np.float64(decay_weight)
                hit = np.nonzero(A[pos:] < th if strict else A[pos:] <= th)[0]
                if not len(hit):
                    break
                i = pos + int(hit[0])
                w, m = float(A[i]), int(bins[i])
                pos = i + 1
        if upto is not None and upto[0] == t:
            return m, w
        out.append((m, w))
    return out


def replay_states(sc, tables=None):
    r, c, b = tables if tables is not None else sc.tables
    dw = math.exp(-sc.decay) if 0.0 < sc.decay < 1.0 else None
    assert dw is not None or sc.decay == 1.0
    per = [replay_slot(sc.trace, r[s], c[s], b[s], dw) for s in range(sc.S)]
    mins = np.array([[per[s][t][0] for s in range(sc.S)] for t in range(sc.n_flush)], dtype=np.uint64)
    weights = np.array([[per[s][t][1] for s in range(sc.S)] for t in range(sc.n_flush)], dtype=np.float64)
    return mins, weights


def row_min(trace, tab, s, skip=()):
    """the smallest A of slot s over the whole stream (fp64), bins in `skip` left out"""
    r, c, b = tab
    best = np.inf
    for bins, f in trace:
        keep = ~np.isin(bins, list(skip)) if len(skip) else slice(None)
        a = A64(r[s, bins], c[s, bins], b[s, bins], f)[keep]
        if len(a):
            best = min(best, float(a.min()))
    return best


def first_seen(trace):
    """{bin: flush of its first occurrence}"""
    seen = {}
    for t, (bins, _f) in enumerate(trace):
        for x in bins.tolist():
            seen.setdefault(x, t)
    return seen


def fp32_screen_argmin(trace_t, r_row, c_row, b_row):
    """what an argmin over the fp32 products of the scan (K32 * rcp32) would pick in one flush: not the device's code, an
    emulation that shows how many planted cases an fp32 order gets wrong"""
    bins, f = trace_t
    k32 = (c_row[bins] * np.exp(b_row[bins] - r_row[bins])).astype(np.float32)
    rcp = (1.0 / f).astype(np.float32)
    return int(bins[int(np.argmin(k32 * rcp))])


def random_spectrum(rng, frac, hi, exclude_tiles=()):
    h = ((rng.random(B) < frac) * rng.integers(1, hi + 1, size=B)).astype(np.uint32)
    for t in exclude_tiles:
        h[t * TILE:(t + 1) * TILE] = 0
    return h


# ---- generator 1: planted near-ties, one flush ----------------------------------------------------------------------------------
def signed_deltas():
    return [d for d in DELTAS] + [-d for d in DELTAS] + [DELTA_OUT, -DELTA_OUT]


@functools.lru_cache(maxsize=None)
def near_ties_single(seed=1):
    """16 slots, one spectrum.  Slot s: bins x and y of different wave tiles with A_x = 1.5 * (row minimum) and
    A_y = A_x * (1 + delta_s): y wins for delta > 0 (A is negative), x otherwise."""
    rng = np.random.default_rng(seed)
    deltas = signed_deltas()
    S = len(deltas)
    spectra = [random_spectrum(rng, 0.3, 30)]
    trace = stream_trace(spectra=spectra)
    tab = base_tables(rng, S)
    sc = Scenario("near_ties_single", S, tab, spectra=spectra)
    sc.trace = trace
    bins, f = trace[0]
    fof = dict(zip(bins.tolist(), f.tolist()))
    sc.info["pairs"] = []
    for s, d in enumerate(deltas):
        while True:
            x, y = (int(v) for v in rng.choice(bins, size=2, replace=False))
            if x // TILE != y // TILE:
                break
        lo = row_min(trace, tab, s)
        assert lo < 0
        tab[1][s, x] = solve_c(mp().mpf(1.5 * lo), tab[0][s, x], tab[2][s, x], fof[x])
        ax = A_mp(tab[0][s, x], tab[1][s, x], tab[2][s, x], fof[x])
        gap = plant_relative(tab, s, y, fof[y], ax, d)
        sc.gaps.append((d, gap))
        sc.winners[(0, s)] = y if d > 0 else x
        sc.info["pairs"].append((x, y))
    return sc


# ---- generator 2: quantised tables, exact ties ---------------------------------------------------------------------------------
R_SET, BR_SET = (0.7, 1.6), (0.0, 0.5)
C_NEG, C_POS = (-1.0, -math.sqrt(2.0)), (1.0, math.sqrt(2.0))
C_TOP = -math.sqrt(3.0)          # a class of its own below every drawn one, for ties between two chosen bins


def quantised_tables(rng, S, p_extra):
    """r, b/r, c from two values each, drawn evenly; a further share p_extra[s] of the bins of slot s is moved into the class
    (r = 0.7, b = 0.35, c = -sqrt 2), the one that wins among bins of equal f (smallest r - b, most negative c)."""
    r = np.empty((S, B)); c = np.empty((S, B)); b = np.empty((S, B))
    for s in range(S):
        win = rng.random(B) < p_extra[s]
        ri = np.where(win, 0, rng.integers(0, 2, size=B))
        bi = np.where(win, 1, rng.integers(0, 2, size=B))
        ci = np.where(win, 1, rng.integers(0, 2, size=B))
        r[s] = np.array(R_SET)[ri]; b[s] = np.array(BR_SET)[bi] * r[s]; c[s] = np.array(C_NEG)[ci]
    return r, c, b


def class_separation(trace, tab, slots):
    """Every distinct (r, b, c, f) that occurs in the stream of `slots`, evaluated at 50 digits; returns (number of classes,
    smallest relative distance between two of them).  c == 0 is one class whatever r, b, f (the value is exactly 0)."""
    r, c, b = tab
    seen = set()
    for bins, f in trace:
        for s in slots:
            q = np.stack([r[s, bins], b[s, bins], c[s, bins], f], axis=1)
            q[q[:, 2] == 0.0] = 0.0
            seen.update(map(tuple, np.unique(q, axis=0).tolist()))
    vals = sorted(A_mp(rr, cc, bb, ff) if cc != 0.0 else mp().mpf(0) for rr, bb, cc, ff in seen)
    gaps = [abs(hi - lo) / max(abs(hi), abs(lo)) for lo, hi in zip(vals[:-1], vals[1:])]
    return len(vals), float(min(gaps))


def tied_tiles(trace_t, tab, s):
    """(bins of flush t that share the flush's smallest A in slot s, number of wave tiles they lie in)"""
    bins, f = trace_t
    a = A64(tab[0][s, bins], tab[1][s, bins], tab[2][s, bins], f)
    tied = bins[a == a.min()]
    return tied, len(np.unique(tied // TILE))


QS = 16
Q_MANY, Q_FEW, Q_POS, Q_ZERO, Q_EDGE, Q_LAST, Q_LANE = (0, 1, 2, 3), (4, 5, 6, 7), 8, 9, 10, 11, 12
LANE_TRIPLES = tuple(j * TILE + 33 for j in (60, 100, 140))   # x of (x, x + 256, x + 512): forced into the quantised spectrum
Q_FEW_BINS = (2, 5, 20, 60)


def _quantised(rng, trace, sc_name, **stream):
    """the slots of both quantised scenarios, over the first flush of `trace`:
    0-3 the winning class in ~30 % of the bins (ties over far more than 64 wave tiles); 4-7 cut down to 2 / 5 / 20 / 60 tied
    bins; 8 all c > 0 (every K >= 0: the rmin side of the bounds); 9 c == 0 in three bins of a positive row (A == 0 wins);
    10 a tie between the last bin of a wave tile and the first of the next; 11 a tie between a bin of the last, partly filled
    tile and one of tile 0; 12 a tie between bins x, x + 256, x + 512: the same position of three wave tiles, which ONE thread of
    the resolve compares (it visits bins cand[i] * 256 + tid, in the order the candidate list happened to be filled); 13-15 as
    drawn."""
    tab = quantised_tables(rng, QS, [0.25] * 4 + [0.0] * 12)
    r, c, b = tab
    sc = Scenario(sc_name, QS, tab, **stream)
    sc.trace = trace
    bins, f = trace[0]
    fmin = f.min()
    low = bins[f == fmin]                                      # the bins a winner can come from
    for s, keep in zip(Q_FEW, Q_FEW_BINS):
        win = low[(r[s, low] == 0.7) & (b[s, low] == 0.35) & (c[s, low] == C_NEG[1])]
        assert len(win) > keep
        drop = np.setdiff1d(bins[(r[s, bins] == 0.7) & (b[s, bins] == 0.35) & (c[s, bins] == C_NEG[1])], rng.choice(win, size=keep, replace=False))
        c[s, drop] = C_NEG[0]
    c[Q_POS] = np.where(c[Q_POS] == C_NEG[0], C_POS[0], C_POS[1])
    c[Q_ZERO] = np.where(c[Q_ZERO] == C_NEG[0], C_POS[0], C_POS[1])
    zero = rng.choice(bins, size=3, replace=False)
    c[Q_ZERO, zero] = 0.0
    sc.info["zero_bins"] = np.sort(zero)
    # two chosen bins of equal f in a class of their own
    fof = dict(zip(bins.tolist(), f.tolist()))
    edge = [(j * TILE - 1, j * TILE) for j in range(1, NTILES) if fof.get(j * TILE - 1) == fmin and fof.get(j * TILE) == fmin]
    assert edge, "no adjacent pair of bins across a tile border with the smallest f: the spectrum must force some"
    lastt = [x for x in range((NTILES - 1) * TILE, B) if fof.get(x) == fmin]
    first = [x for x in range(0, TILE) if fof.get(x) == fmin]
    assert lastt and first
    sc.info["edge"] = edge[len(edge) // 2]
    sc.info["last"] = (first[-1], lastt[0])
    lane = [(x, x + TILE, x + 2 * TILE) for x in LANE_TRIPLES if all(fof.get(x + i * TILE) == fmin for i in range(3))]
    assert lane, "no triple x, x + 256, x + 512 with the smallest f"
    sc.info["lane"] = lane[0]
    for s, pair in ((Q_EDGE, sc.info["edge"]), (Q_LAST, sc.info["last"]), (Q_LANE, sc.info["lane"])):
        for x in pair:
            r[s, x], b[s, x], c[s, x] = 0.7, 0.35, C_TOP
        sc.winners[(0, s)] = pair[0]
    sc.winners[(0, Q_ZERO)] = int(sc.info["zero_bins"][0])
    return sc


def forced_bins():
    """bins a quantised spectrum always holds with count 1: both sides of some tile borders, some of tile 0 and of the last tile"""
    js = (3, 40, 77, 120, 150, 190)
    out = [j * TILE - 1 for j in js] + [j * TILE for j in js] + [5, 77, 200] + [B - 1, B - 100, (NTILES - 1) * TILE + 7]
    out += [x + i * TILE for x in LANE_TRIPLES for i in range(3)]
    return np.array(sorted(out))


@functools.lru_cache(maxsize=None)
def quantised_single(seed=2):
    """One spectrum of ~2500 bins with count 1 (so that most estimates are exactly 1) plus a few 2s and 3s."""
    rng = np.random.default_rng(seed)
    h = np.zeros(B, dtype=np.uint32)
    h[rng.choice(B, size=2500, replace=False)] = rng.choice([1, 1, 1, 1, 1, 1, 2, 3], size=2500)
    h[forced_bins()] = 1
    spectra = [h]
    trace = stream_trace(spectra=spectra)
    return _quantised(rng, trace, "quantised_single", spectra=spectra)


# ---- generator 3: later flushes at the weight's margin -------------------------------------------------------------------------
def _margins(name, seed, plan, pow2=False, bound_above=False):
    """Five flushes.  Flush 0 sets every slot's weight through one bin x (A_x = 1.5 * row minimum, negative); flushes 1-3 repeat
    the same spectrum (estimates grow, nothing can replace: the scan prunes nearly every tile); flush 4 brings a bin z no earlier
    spectrum held, alone in its wave tile, with the same estimate as x had in flush 0 and A_z = w * (1 + plan[s]).
    delta > 0: z replaces; delta < 0: it does not; plan[s] == "dup": z is the exact duplicate of x (same r, c, b, f), strict <
    keeps x.  K_z, K_x are the most negative K of their rows, and z is the only element of its tile, so the scan's bound for that
    tile is K32_z * rcp32(f_z): within fp32 rounding of the weight itself.
    pow2: the common estimate of x and z is a power of two, so that rcp32(f) is exact however the device forms it.
    bound_above: A_x is moved (1.5 ... 1.8 x the row minimum) until that bound lies ABOVE the weight by at least 1e-9 relative,
    in every slot (scan_bound_excess): without the 1e-5 band k_scan_test would not read z's tile for any row of a slot group."""
    rng = np.random.default_rng(seed)
    S = len(plan)
    zt = 101                                                    # z's wave tile: empty in every spectrum but for z
    z = zt * TILE + 17
    old = random_spectrum(rng, 0.3, 30, exclude_tiles=(zt,))
    present = np.nonzero(old)[0]
    x, late_bins = 0, None

    def spectra_for(cx, cz):
        o = old.copy(); o[x] = cx
        late = np.zeros(B, dtype=np.uint32); late[late_bins] = old[late_bins]; late[z] = cz
        return [o, o.copy(), o.copy(), o.copy(), late]

    def f_of(trace, t, bin_):
        bins, f = trace[t]
        return float(f[np.nonzero(bins == bin_)[0][0]])
    # f_x (flush 0) = cx + the smallest counter under x in front of it, f_z (flush 4) likewise: neither base depends on cx
    # unless x and z share a counter, so cx follows from one trial trace; an x that does share one is passed over
    cz = 50
    for x in (int(v) for v in present[len(present) // 3:]):
        late_bins = rng.choice(np.setdiff1d(present, [x]), size=700, replace=False)
        tr = stream_trace(spectra=spectra_for(1, cz))
        if pow2:                                                # f_z = cz + what lies under z: make it 64, 128, ...
            base = int(f_of(tr, 4, z)) - cz
            cz = (64 << max(0, (base // 64).bit_length())) - base
            tr = stream_trace(spectra=spectra_for(1, cz))
        cx = int(f_of(tr, 4, z) - (f_of(tr, 0, x) - 1))
        spectra = spectra_for(cx, cz)
        tr = stream_trace(spectra=spectra)
        if f_of(tr, 4, z) == f_of(tr, 0, x):
            break
    fx, fz = f_of(tr, 0, x), f_of(tr, 4, z)
    assert fx == fz, (fx, fz)
    tab = base_tables(rng, S)
    r, c, b = tab
    sc = Scenario(name, S, tab, spectra=spectra)
    sc.trace = tr
    sc.info.update(x=x, z=z, fx=fx, dups=[s for s in range(S) if plan[s] == "dup"], deltas={})
    for s in range(S):
        lo = row_min(tr, tab, s, skip=(x, z))
        assert lo < 0
        for t in range(4):
            sc.winners[(t, s)] = x
        for i in range(300 if bound_above else 1):
            c[s, x] = solve_c(mp().mpf(1.5 * (1 + 1e-3 * i) * lo), r[s, x], b[s, x], fx)
            ax = A_mp(r[s, x], c[s, x], b[s, x], fx)
            if plan[s] == "dup":
                r[s, z], c[s, z], b[s, z] = r[s, x], c[s, x], b[s, x]
            else:
                gap = plant_relative(tab, s, z, fz, ax, plan[s])
            if not bound_above or scan_bound_excess(sc, s) >= 1e-9:
                break
        else:
            raise AssertionError(f"slot {s}: no A_x whose fp32 tile bound lies above the weight")
        if plan[s] == "dup":
            sc.winners[(4, s)] = x
            continue
        sc.gaps.append((plan[s], gap))
        sc.info["deltas"][s] = plan[s]
        sc.winners[(4, s)] = z if plan[s] > 0 else x
    return sc


@functools.lru_cache(maxsize=None)
def margins(seed=3):
    """slots 0-6 delta > 0, 7-13 delta < 0 (DELTAS), 14 the duplicate, 15 delta = +2e-5"""
    return _margins("margins", seed, list(DELTAS) + [-d for d in DELTAS] + ["dup", DELTA_OUT])


SCAN_ROWS = 8                    # slots per group of k_scan_test: a wave tile is read if ANY row of the group lets it pass


@functools.lru_cache(maxsize=None)
def scan_margin(seed=7):
    """The pruning margin of k_scan_test.  Its verdict is one bit per (group of 8 slots, wave tile), so the band is only needed
    where EVERY row of a group has the fp32 bound of z's tile above its weight.  Both groups here are built that way (gaps
    below fp32 resolution, negative gaps, the duplicate; A_x moved until the rounding of K32_z falls on the right side), and
    each holds rows where z must replace: without the band the tile is never read and those rows keep x."""
    return _margins("scan_margin", seed, [1e-12, 1e-10, 1e-9, 3e-8, -1e-12, -1e-9, "dup", -2e-7,
                                           1e-10, -1e-10, 3e-8, -3e-8, "dup", 1e-9, -1e-6, -9e-6], pow2=True, bound_above=True)


def scan_bound_fp32(sc, s):
    """k_scan_test's bound for z's tile in flush 4 of a margins scenario, as the device forms it: (double)K32 * (double)rcp32"""
    r, c, b = sc.tables
    z = sc.info["z"]
    k32 = np.float32(c[s, z] * np.exp(b[s, z] - r[s, z]))
    return float(np.float64(k32) * np.float64(np.float32(1.0 / sc.info["fx"])))


def scan_bound_excess(sc, s):
    """(bound - w) / |w| for z's tile in flush 4: w = A_x in fp64, the slot's weight since flush 0.  > 0: only the band lets
    the row pass.  The bound moves in steps of fp32 rounding (~1e-8 ... 1e-7 of w); w is known to ~1e-15."""
    r, c, b = sc.tables
    x = sc.info["x"]
    w = float(A64(r[s, x], c[s, x], b[s, x], sc.info["fx"]))
    return (scan_bound_fp32(sc, s) - w) / abs(w)


# ---- generator 4: multi-interval batches from reads ----------------------------------------------------------------------------
READ_LEN = 150


def synth_reads(first, n):
    from hulk_amd import synth
    return synth.reads_numpy(first, n, READ_LEN)


@functools.lru_cache(maxsize=None)
def batches_from_reads(seed=4, interval=150, n_int=6):
    """Six intervals of reads, tables chosen from the trace.  16 slots:
    0, 1   an exact duplicate in intervals 0 and 2: y is absent from intervals 0 and 1, f_2[y] == f_0[x], same (r, c, b); y < x
           in bin order (slot 0) or y > x (slot 1): the earlier interval wins either way
    2-15   near-ties (both signs of every gap) between a bin that first occurs in one interval and one that first occurs in
           another, the pair's order in the stream alternating"""
    rng = np.random.default_rng(seed)
    reads = synth_reads(0, interval * n_int)
    stream = dict(reads=reads, interval=interval, n_int=n_int)
    trace = stream_trace(**stream)
    S = 16
    tab = base_tables(rng, S)
    r, c, b = tab
    sc = Scenario("batches_from_reads", S, tab, **stream)
    sc.trace = trace
    seen = first_seen(trace)
    f_first = {}                                                # {bin: f at its first occurrence}
    for t, (bins, f) in enumerate(trace):
        for x, v in zip(bins.tolist(), f.tolist()):
            if seen[x] == t:
                f_first[x] = v
    new_in = [np.array(sorted(x for x, t0 in seen.items() if t0 == t)) for t in range(n_int)]
    final = {}
    used = set()

    def pick(t, cond=lambda x: True):
        for _ in range(10000):
            x = int(rng.choice(new_in[t]))
            if x not in used and cond(x):
                used.add(x)
                return x
        raise AssertionError("no bin to pick")

    def plant_x(s, x):
        lo = row_min(trace, tab, s)
        assert lo < 0
        c[s, x] = solve_c(mp().mpf(1.5 * lo), r[s, x], b[s, x], f_first[x])
        return A_mp(r[s, x], c[s, x], b[s, x], f_first[x])
    for s in (0, 1):
        x = pick(0, lambda v: TILE * 20 < v < B - TILE * 20)
        y = pick(2, lambda v: f_first[v] == f_first[x] and v // TILE != x // TILE and ((v < x) if s == 0 else (v > x)))
        plant_x(s, x)
        r[s, y], c[s, y], b[s, y] = r[s, x], c[s, x], b[s, x]
        final[s] = x
        sc.info.setdefault("dups", []).append((x, y))
    ds = [d for d in DELTAS] + [-d for d in DELTAS]
    for i, d in enumerate(ds):
        s = 2 + i
        tx, ty = [(0, 3), (4, 1), (1, 2), (5, 0), (2, 4)][i % 5]
        x = pick(tx)
        y = pick(ty, lambda v: v // TILE != x // TILE)
        ax = plant_x(s, x)
        sc.gaps.append((d, plant_relative(tab, s, y, f_first[y], ax, d)))
        final[s] = y if d > 0 else x
    for s, x in final.items():
        sc.winners[(n_int - 1, s)] = x
    return sc


@functools.lru_cache(maxsize=None)
def quantised_from_reads(seed=5, interval=40, n_int=4):
    """Quantised tables under reads: small intervals (about 1100 bins each, nearly all with estimate 1 in interval 0), so the
    exact ties of the winning class span many wave tiles of interval 0 AND recur in the later intervals of the batch with new
    bins: the earliest (interval, bin) must win in the merged resolve and in every per-interval snapshot."""
    rng = np.random.default_rng(seed)
    stream = dict(reads=synth_reads(100000, interval * n_int), interval=interval, n_int=n_int)
    trace = stream_trace(**stream)
    tab = quantised_tables(rng, QS, [0.4] * 4 + [0.0] * 12)
    sc = Scenario("quantised_from_reads", QS, tab, **stream)
    sc.trace = trace
    return sc


# ---- generator 5: concept drift -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def drift(decay, seed=6, interval=150, n_int=6):
    """Reads, concept drift: if A < w / decayWeight.  Every planted slot first gets an anchor (a bin that first occurs in interval
    0, at 3 * row minimum: from then on no drawn element comes near the threshold), then elements at
    A = (w_before / decayWeight) * (1 + delta), w_before from the one-slot replay: delta > 0 replaces when w is negative.
      slots 0-6   two triggers in ONE wave tile of interval 1 (a clear one at 1.5 x the threshold, then one at the margin, planted
                  against the weight the first leaves), then a non-trigger at the margin in the same tile
      slots 7-9   triggers in consecutive wave tiles of interval 2 (clear, then at the margin), a non-trigger at the margin later
      slots 10-12 a trigger at the margin late in interval 2, then one in the first wave tile of the NEXT interval (3)
    (A margin trigger is only ever followed by margin NON-triggers inside its interval: a later trigger would fire whichever way
    the earlier decision went and hide it from the snapshot at the interval's end.)
      slot 13     positive weights: every c > 0, the anchor at 1e-3 * row minimum; then w / decayWeight > w and a LARGER A replaces;
                  in the last interval two bins with c == 0: A == w / decayWeight == 0 exactly for the second (strict <)
      slots 14,15 as drawn (the first element of the stream meets the threshold MaxFloat64 / decayWeight = +Inf in every slot)
    info["planted"]: [(slot, flush, position in the flush, bin, delta)] for the sensitivity check."""
    rng = np.random.default_rng(seed + int(decay * 1000))
    stream = dict(reads=synth_reads(200000, interval * n_int), interval=interval, n_int=n_int)
    trace = stream_trace(decay=decay, **stream)
    dw = math.exp(-decay)
    S = 16
    tab = base_tables(rng, S)
    r, c, b = tab
    sc = Scenario(f"drift_{decay}", S, tab, decay=decay, **stream)
    sc.trace = trace
    seen = first_seen(trace)
    pos_of = [dict(zip(bins.tolist(), range(len(bins)))) for bins, _f in trace]
    planted = []
    used = set()

    def new_bins(t, tiles=None):
        bins = trace[t][0]
        ok = np.array([seen[x] == t and x not in used for x in bins.tolist()])
        if tiles is not None:
            ok &= np.isin(bins // TILE, tiles)
        return bins[ok]

    def anchor(s, factor):
        x = int(new_bins(0)[len(new_bins(0)) // 2 + s]); used.add(x)
        lo = row_min(trace, tab, s)
        c[s, x] = solve_c(mp().mpf(factor * lo), r[s, x], b[s, x], trace[0][1][pos_of[0][x]])

    def plant(s, t, x, d):
        """margin element: A = threshold * (1 +- |d|), d > 0 replaces.  d = None: a clear trigger at 1.5 x the threshold (w < 0)"""
        used.add(x)
        p = pos_of[t][x]
        _m, wb = replay_slot(trace, r[s], c[s], b[s], dw, upto=(t, p))
        th = mp().mpf(wb) / mp().mpf(dw)
        if d is None:
            assert wb < 0
            c[s, x] = solve_c(th * 1.5, r[s, x], b[s, x], trace[t][1][p])
            return
        gap = plant_relative(tab, s, x, trace[t][1][p], th, d if wb < 0 else -d)
        sc.gaps.append((d if wb < 0 else -d, gap))
        planted.append((s, t, p, x, d))

    def tile_with(t, need, after_tile=0):
        """a wave tile (>= after_tile) of flush t that holds at least `need` bins first seen in t"""
        for tile in range(after_tile, NTILES):
            if len(new_bins(t, [tile])) >= need:
                return tile
        raise AssertionError("no such tile")
    dd = list(DRIFT_DELTAS)
    sc.info["two_in_one_tile"], sc.info["consecutive"] = [], []
    for s in range(7):
        anchor(s, 3.0)
        tile = tile_with(1, 3, after_tile=10 + 9 * s)
        xa, x1, x2 = (int(v) for v in new_bins(1, [tile])[:3])
        plant(s, 1, xa, None)
        plant(s, 1, x1, dd[s])
        plant(s, 1, x2, -dd[(s + 3) % 7])
        sc.info["two_in_one_tile"].append((s, xa, x1))
    for s in range(7, 10):
        anchor(s, 3.0)
        tile = next(tl for tl in range(30 + 20 * (s - 7), NTILES - 2) if len(new_bins(2, [tl])) and len(new_bins(2, [tl + 1])))
        xa, x1 = int(new_bins(2, [tile])[-1]), int(new_bins(2, [tile + 1])[0])
        plant(s, 2, xa, None)
        plant(s, 2, x1, dd[s - 7])
        plant(s, 2, int(new_bins(2, list(range(tile + 2, NTILES)))[3]), -dd[s - 5])
        sc.info["consecutive"].append((s, xa, x1))
    for s in range(10, 13):
        anchor(s, 3.0)
        plant(s, 2, int(new_bins(2, list(range(150, NTILES)))[-1 - s]), dd[s - 10])
        plant(s, 3, int(new_bins(3, [0])[0]), dd[s - 8] * (1 if s != 11 else -1))
    s = 13
    c[s] = np.abs(c[s]) + 0.5
    x = int(new_bins(0)[7]); used.add(x)
    c[s, x] = solve_c(mp().mpf(1e-3 * row_min(trace, tab, s)), r[s, x], b[s, x], trace[0][1][pos_of[0][x]])
    plant(s, 1, int(new_bins(1)[40]), 1e-9)           # (w > 0: plant() turns the sign so that d > 0 still means "replaces")
    plant(s, 2, int(new_bins(2)[300]), -3e-8)
    plant(s, 4, int(new_bins(4)[100]), 2e-7)
    # A == 0 twice: the one exact equality with the threshold that needs no bit of f.  Two bins that first occur in the last
    # interval get c = 0: the first meets w > 0 and sets w = 0; for the second A = 0 and w / decayWeight = 0 on either side,
    # whatever f is: the strict < keeps the first.  (Every other c of the row is positive, so nothing else can follow.)
    z0, z1 = (int(v) for v in new_bins(n_int - 1)[[50, 200]])
    assert z0 < z1 and z0 // TILE != z1 // TILE
    c[s, z0] = c[s, z1] = 0.0
    sc.info["zero_pair"] = (n_int - 1, z0, z1)
    sc.winners[(n_int - 1, s)] = z0
    sc.info["planted"] = planted
    return sc


def flip_planted(sc, which):
    """the tables of a drift scenario with the gap of planted element `which` mirrored (delta -> -delta)"""
    s, t, p, x, _d = sc.info["planted"][which]
    r, c, b = (a.copy() for a in sc.tables)
    dw = math.exp(-sc.decay)
    _m, wb = replay_slot(sc.trace, r[s], c[s], b[s], dw, upto=(t, p))
    th = mp().mpf(wb) / mp().mpf(dw)
    now = A_mp(r[s, x], c[s, x], b[s, x], sc.trace[t][1][p]) / th - 1
    plant_relative((r, c, b), s, x, sc.trace[t][1][p], th, -float(now))
    return r, c, b


# ---- the device side --------------------------------------------------------------------------------------------------------------
def gpu_states(sc, tables=None, flags=0, batch=0, work_lanes=0, snapshots=0, slot_begin=0, slot_count=0):
    """Run a scenario through libhulkhip with external tables.  Returns (mins[n][S], weights[n][S], scan_stats per flush or None):
    spectra: the sketch after every hulk_flush;  reads: the per-interval snapshots if snapshots == 1, else the final sketch alone."""
    import hulk_amd
    from hulk_amd import _lib
    g = hulk_amd.GpuSketcher(K, W, sc.S, sc.interval, sc.decay, B, cws_source=_lib.HULK_CWS_EXTERNAL, flags=flags, batch=batch,
                             work_lanes=work_lanes, snapshots=snapshots, snapshot_capacity=64 if snapshots else 0,
                             slot_begin=slot_begin, slot_count=slot_count)
    try:
        g.set_cws_tables(*(tables if tables is not None else sc.tables))
        ms, ws, stats = [], [], []
        if sc.spectra is not None:
            for h in sc.spectra:
                g.add_histogram(h); g.flush()
                m, w = g.sketch(); ms.append(m); ws.append(w); stats.append(g.scan_stats())
        else:
            g.add_reads(*sc.reads)
            g.finish()
            if snapshots:
                info, m, w = g.snapshots()
                assert [i["ordinal"] for i in info] == list(range(1, sc.n_int + 1))
                ms, ws = list(m), list(w)
            fm, fw = g.sketch()
            if snapshots:
                assert np.array_equal(fm, ms[-1]) and np.array_equal(fw.view(np.uint64), ws[-1].view(np.uint64))
            else:
                ms, ws = [fm], [fw]
            stats = None
        cms = g.cms()
    finally:
        g.close()
    return np.stack(ms), np.stack(ws), stats, cms
