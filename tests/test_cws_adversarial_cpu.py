"""The CPU half of the adversarial CWS tests: the seeded generators of tests/cws_adversarial.py, their certificates, and the
oracle against the one-slot numpy replay on every scenario tests/test_gpu_cws_adversarial.py runs on the device.

Asserted here, before any GPU sees the inputs:
  * every planted gap, re-evaluated at 50 digits from the rounded fp64 table entries, is within 1 % of its design and at least
    1e-12 (see the module docstring of cws_adversarial for why 1e-12 is safe across libms);
  * the distinct (r, b, c, f) classes of the quantised tables are at least 1e-9 apart;
  * at least four slots tie over more than 64 wave tiles, others over 2 to 64;
  * in the scan_margin scenario the fp32 bound of z's tile lies above the weight in EVERY row of both 8-slot groups of
    k_scan_test (its verdict is per group), and each group holds rows where z replaces;
  * with concept drift, a replay with <= in place of < ends on another bin (A == 0 twice), and mirroring the gap of any one planted element changes a per-interval state the GPU test reads;
  * the oracle equals the replay (mins exactly, weights to 1e-12) and picks every designed winner.
"""
import math

import numpy as np
import pytest

import cws_adversarial as adv


def assert_gaps(sc, n):
    assert len(sc.gaps) == n
    for designed, realised in sc.gaps:
        print(f"{sc.name}: gap designed {designed:+.3e} realised {realised:+.6e}")
        assert adv.gap_ok(realised, designed), (designed, realised)


def assert_oracle_is_replay(sc):
    om, ow = adv.oracle_states(sc)
    rm, rw = adv.replay_states(sc)
    assert np.array_equal(om, rm), f"{sc.name}: oracle and replay disagree on {int((om != rm).sum())} (flush, slot) mins"
    assert np.allclose(ow, rw, rtol=1e-12, atol=0)
    for (t, s), x in sc.winners.items():
        assert om[t, s] == x, f"{sc.name}: flush {t} slot {s}: the oracle has bin {om[t, s]}, designed {x}"
    return om, ow


def test_trace_and_table_setter_of_the_oracle():
    """the trace is the AddElement stream (bins ascending inside a flush, estimates = count-min as the replayed counters give them)
    and set_cws_tables is what the sketch follows"""
    from oracle import pyorc
    rng = np.random.default_rng(0)
    S = 3
    spectra = [adv.random_spectrum(rng, 0.05, 9), adv.random_spectrum(rng, 0.05, 9)]
    tr = adv.stream_trace(spectra=spectra)
    depth, width = pyorc.cms_geometry()
    ctr = np.zeros((depth, width))
    for h, (bins, f) in zip(spectra, tr):
        assert np.array_equal(bins, np.nonzero(h)[0])
        for x, v, fx in zip(bins.tolist(), h[bins].tolist(), f.tolist()):
            pos = [pyorc.jump((x + d * x) & 0xFFFFFFFFFFFFFFFF, width) for d in range(depth)]
            for d in range(depth):
                ctr[d, pos[d]] += v
            assert fx == min(ctr[d, pos[d]] for d in range(depth))
    tab = adv.base_tables(rng, S)
    sc = adv.Scenario("setter", S, tab, spectra=spectra)
    sc.trace = tr
    assert_oracle_is_replay(sc)
    o = pyorc.Sketcher(adv.K, adv.W, S, adv.B)
    assert not np.array_equal(o.cws()[0], tab[0])
    o.set_cws_tables(*tab)
    assert all(np.array_equal(a, b) for a, b in zip(o.cws(), tab))
    o.close()


def test_drift_trace_scales_per_element():
    """with concept drift cms_add scales every counter per element: the trace must carry those estimates"""
    from oracle import pyorc
    rng = np.random.default_rng(1)
    decay = 0.5
    spectra = [adv.random_spectrum(rng, 0.02, 5)]
    (bins, f), = adv.stream_trace(decay=decay, spectra=spectra)
    depth, width = pyorc.cms_geometry()
    ctr = np.zeros((depth, width))
    dw = math.exp(-decay)
    for x, v, fx in list(zip(bins.tolist(), spectra[0][bins].tolist(), f.tolist()))[:300]:
        ctr *= dw
        pos = [pyorc.jump((x + d * x) & 0xFFFFFFFFFFFFFFFF, width) for d in range(depth)]
        for d in range(depth):
            ctr[d, pos[d]] += v
        assert fx == min(ctr[d, pos[d]] for d in range(depth))


def test_planted_near_ties_one_flush():
    sc = adv.near_ties_single()
    assert_gaps(sc, 16)
    assert all(x // adv.TILE != y // adv.TILE for x, y in sc.info["pairs"])
    assert_oracle_is_replay(sc)
    r, c, b = sc.tables
    wrong = sum(adv.fp32_screen_argmin(sc.trace[0], r[s], c[s], b[s]) != sc.winners[(0, s)] for s in range(sc.S))
    print(f"near_ties_single: an fp32 argmin picks the wrong bin in {wrong} of {sc.S} slots")
    assert wrong >= 1, "every near-tie is resolved by the fp32 order: the scenario does not need the fp64 re-evaluation"


def test_quantised_tables_one_flush():
    sc = adv.quantised_single()
    n, sep = adv.class_separation(sc.trace, sc.tables, range(sc.S))
    print(f"quantised_single: {n} classes, smallest relative distance {sep:.3e}")
    assert sep >= 1e-9
    om, _ = assert_oracle_is_replay(sc)
    tiles = [adv.tied_tiles(sc.trace[0], sc.tables, s)[1] for s in range(sc.S)]
    print("quantised_single: wave tiles of the tied minimum per slot:", tiles)
    assert all(tiles[s] > 64 for s in adv.Q_MANY)
    assert all(2 <= tiles[s] <= 64 for s in adv.Q_FEW)
    for s in range(sc.S):                                          # the earliest of the tied bins
        assert om[0, s] == adv.tied_tiles(sc.trace[0], sc.tables, s)[0].min()
    r, c, b = sc.tables
    bins = sc.trace[0][0]
    assert (c[adv.Q_POS] > 0).all() and (c[adv.Q_ZERO][np.setdiff1d(bins, sc.info["zero_bins"])] > 0).all()
    assert c[adv.Q_ZERO, om[0, adv.Q_ZERO]] == 0.0
    x, y = sc.info["edge"]
    assert y == x + 1 and y % adv.TILE == 0
    assert set(adv.tied_tiles(sc.trace[0], sc.tables, adv.Q_EDGE)[0].tolist()) == {x, y}
    x, y = sc.info["last"]
    assert x < adv.TILE and (adv.NTILES - 1) * adv.TILE <= y < adv.B and adv.B % adv.TILE != 0
    assert set(adv.tied_tiles(sc.trace[0], sc.tables, adv.Q_LAST)[0].tolist()) == {x, y}
    # three tied bins at the same position of three wave tiles: one thread of the per-interval resolve decides among them
    x, y, z = sc.info["lane"]
    assert (y, z) == (x + adv.TILE, x + 2 * adv.TILE) and om[0, adv.Q_LANE] == x
    assert adv.tied_tiles(sc.trace[0], sc.tables, adv.Q_LANE)[0].tolist() == [x, y, z]


def check_margins(sc, ngaps):
    assert_gaps(sc, ngaps)
    om, ow = assert_oracle_is_replay(sc)
    x, z = sc.info["x"], sc.info["z"]
    r, c, b = sc.tables
    assert all(z not in sc.trace[t][0] for t in range(4)) and z in sc.trace[4][0]
    assert (sc.trace[4][0] // adv.TILE == z // adv.TILE).sum() == 1          # alone in its wave tile
    assert (ow[3] < 0).all()
    k = c * np.exp(b - r)
    for s in range(sc.S):
        assert set(np.argsort(k[s])[:2].tolist()) == {x, z}                   # the two most negative K of the row
    for s in sc.info["dups"]:
        assert (r[s, z], c[s, z], b[s, z]) == (r[s, x], c[s, x], b[s, x]) and om[4, s] == x and ow[4, s] == ow[3, s]
    return sc, om, ow


def test_margins_of_later_flushes():
    """(whether k_scan_test needs its band here is not asked: its verdict is per group of 8 slots, and in both groups of this
    scenario some row passes without it — that margin is test_scan_margin_needs_the_band_in_every_row_of_a_group's)"""
    sc, _om, _ow = check_margins(adv.margins(), 15)
    assert len(sc.info["dups"]) == 1


def test_scan_margin_needs_the_band_in_every_row_of_a_group():
    """k_scan_test reads a wave tile if ANY of a group's 8 rows has bound <= w + band.  Here, for z's tile in flush 4, EVERY row
    of both groups has its fp32 bound above w (by >= 1e-9 of w: fp32 rounding moves it in steps of ~1e-8 ... 1e-7, fp64 noise
    is 1e-15; the estimate is a power of two, so its reciprocal is exact) and each group holds rows, inside the band, where
    z replaces: a scan without the band passes the tile over and those rows keep x."""
    sc, om, ow = check_margins(adv.scan_margin(), 14)
    fx = sc.info["fx"]
    assert fx >= 64 and math.log2(fx) == int(math.log2(fx))
    for g in range(0, sc.S, adv.SCAN_ROWS):
        rows = range(g, g + adv.SCAN_ROWS)
        ex = [adv.scan_bound_excess(sc, s) for s in rows]
        print(f"scan_margin: group {g // adv.SCAN_ROWS}: (bound - w) / |w| per row:", " ".join(f"{e:.2e}" for e in ex))
        assert all(e >= 1e-9 for e in ex)
        for s in rows:
            assert ow[3, s] == adv.A64(sc.tables[0][s, sc.info["x"]], sc.tables[1][s, sc.info["x"]], sc.tables[2][s, sc.info["x"]], fx)
        replaced = [s for s in rows if om[4, s] == sc.info["z"]]
        assert len(replaced) >= 3 and all(sc.info["deltas"].get(s, 0) > 0 for s in replaced)
        assert all(ex[s - g] <= 0.9e-5 for s in replaced)         # ... and the band does let them pass


def test_batches_from_reads():
    sc = adv.batches_from_reads()
    assert_gaps(sc, 14)
    om, _ = assert_oracle_is_replay(sc)
    for s, (x, y) in enumerate(sc.info["dups"]):
        assert all(y not in sc.trace[t][0] for t in (0, 1)) and y in sc.trace[2][0] and x in sc.trace[0][0]
        assert ((y < x) if s == 0 else (y > x)) and om[-1, s] == x
    assert all(len(bins) >= 0.01 * adv.B for bins, _f in sc.trace)


def test_quantised_tables_from_reads():
    sc = adv.quantised_from_reads()
    n, sep = adv.class_separation(sc.trace, sc.tables, range(sc.S))
    print(f"quantised_from_reads: {n} classes, smallest relative distance {sep:.3e}")
    assert sep >= 1e-9
    om, ow = assert_oracle_is_replay(sc)
    tiles = [adv.tied_tiles(sc.trace[0], sc.tables, s)[1] for s in range(sc.S)]
    print("quantised_from_reads: wave tiles of interval 0's tied minimum per slot:", tiles)
    assert sum(t > 64 for t in tiles) >= 4
    # the tie recurs in later intervals (new bins with the same estimate): the weight never moves again, the min stays
    again = 0
    for s in range(sc.S):
        for t in range(1, sc.n_int):
            bins, f = sc.trace[t]
            a = adv.A64(sc.tables[0][s, bins], sc.tables[1][s, bins], sc.tables[2][s, bins], f)
            if a.min() == ow[0, s]:
                again += 1
                assert bins[a == a.min()].min() != om[0, s]
    print(f"quantised_from_reads: (slot, later interval) pairs that tie with interval 0's winner: {again}")
    assert again >= 8
    assert (om == om[0]).all() and (ow == ow[0]).all()


@pytest.mark.parametrize("decay", [0.02, 0.5])
def test_drift_plants_are_sensitive(decay):
    sc = adv.drift(decay)
    for designed, realised in sc.gaps:
        assert abs(realised / designed - 1) < 0.01 and abs(realised) >= 1e-10 and (realised > 0) == (designed > 0)
    assert len(sc.gaps) == len(sc.info["planted"]) == 7 * 2 + 3 * 2 + 3 * 2 + 3
    om, ow = assert_oracle_is_replay(sc)
    rm, rw = adv.replay_states(sc)
    # the positions the plan names are what the oracle went through
    for s, xa, x1 in sc.info["two_in_one_tile"]:
        assert xa // adv.TILE == x1 // adv.TILE and xa < x1 and om[1, s] == x1
    for s, xa, x1 in sc.info["consecutive"]:
        assert x1 // adv.TILE == xa // adv.TILE + 1 and om[2, s] == x1
    assert (ow[:5, 13] > 0).all() and ow[1, 13] > ow[0, 13]       # positive weights: a larger A replaced
    t0, z0, z1 = sc.info["zero_pair"]                              # A == 0 twice: the second equals the threshold 0 / decayWeight
    assert t0 == sc.n_int - 1 and all(z not in sc.trace[t][0] for t in range(t0) for z in (z0, z1))
    p0, p1 = (int(np.nonzero(sc.trace[t0][0] == z)[0][0]) for z in (z0, z1))
    assert p0 < p1 and om[t0, 13] == z0 and om[t0 - 1, 13] != z0 and ow[t0, 13] == 0.0 and not np.signbit(ow[t0, 13])
    le = adv.replay_slot(sc.trace, *(a[13] for a in sc.tables), math.exp(-decay), strict=False)[-1][0]
    assert le == z1, "with <= in place of < the second A == 0 would replace the first: the case does not show the strict test"
    first = int(sc.trace[0][0][0])
    r, c, b = sc.tables
    a0 = adv.A64(r[:, first], c[:, first], b[:, first], sc.trace[0][1][0])
    assert (a0 > 0).any(), "no slot whose first element is positive: the +Inf threshold is not shown to accept everything"
    for i, (s, t, p, x, d) in enumerate(sc.info["planted"]):
        assert (om[t, s] == x) == (d > 0), (i, s, t, x, d)
        fm, fw = adv.replay_states(sc, adv.flip_planted(sc, i))
        differs = (fm != rm) | (fw != rw)
        assert differs[:, s].any(), f"planted element {i} (slot {s}, interval {t}, bin {x}): mirroring its gap changes no state"
