"""Sketch snapshots scored against a panel of reference sketches where they are recorded (hulk_set_panel, k_snap_panel).

The yardstick throughout is oracle.pyorc.smash_matrix — HULKdata.GetDistance for all pairs, the literal CPU restatement that
tests/test_gpu_smash.py uses: the snapshots and the panel are stacked, [snapshots; panel], it is called once, and the block
[:m, m:] is what role "row" (the snapshot is the subject) must give, [m:, :m].T what role "column" (the panel sketch is the
subject) must give — compared bit for bit on the uint64 view, NaNs included.

The in-stream tests reuse the moving stream of tests/test_gpu_snapshots.py (local copies of its helpers): K = 15, W = 9, I = 400,
40 intervals, "nodrift" S = 256 and "decay" S = 64."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import pyorc

pytestmark = pytest.mark.gpu

K, W, I, N_INT, L = 15, 9, 400, 40, 150
MAXF = 1.7976931348623157e308
CONFIGS = {"nodrift": dict(S=256, decay=1.0, min_moves=8), "decay": dict(S=64, decay=0.02, min_moves=30)}
VARIANTS = [("jaccard", "row"), ("jaccard", "column"), ("weightedjaccard", "row"), ("weightedjaccard", "column")]
N_PANEL = 37


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def yardsticks(sm, sw, pm, pw, metric):
    """one call of the yardstick over [snapshots; panel] -> {"row": ..., "column": ...}"""
    m = len(sm)
    full = pyorc.smash_matrix(np.vstack([sm, pm]), np.vstack([sw, pw]), metric)
    return {"row": np.ascontiguousarray(full[:m, m:]), "column": np.ascontiguousarray(full[m:, :m].T)}


def yardstick(sm, sw, pm, pw, metric, role):
    return yardsticks(sm, sw, pm, pw, metric)[role]


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} distances differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r} ({int(bits(got)[tuple(bad[0])]):#x}), want {want[tuple(bad[0])]!r} ({int(bits(want)[tuple(bad[0])]):#x})"


# ---- 1. the kernel at planted shapes (hulk_panel_distances) ------------------------------------------------------------------
def make_sketches(rng, n, s, base, bins=194481):
    """tests/test_gpu_smash.py's generator with the base shared between the two sides, so that equal slots exist across them"""
    mins = np.empty((n, s), dtype=np.uint64)
    for i in range(n):
        keep = rng.random(s) < (0.2 + 0.6 * rng.random())
        mins[i] = np.where(keep, base, rng.integers(0, bins, size=s).astype(np.uint64))
    weights = -rng.gamma(2.0, 1e-3, size=(n, s))            # histosketch weights are mostly negative
    weights[rng.random((n, s)) < 0.05] *= -1                # ... some positive
    return mins, weights


@pytest.mark.parametrize("s", [1, 33, 50, 512])
def test_kernel_at_planted_shapes(s):
    """m: one snapshot, a few, a full flush of 16, a second launch (17), a third (33); P: a tail lane (1, 2, 63), a full wave (64),
    a second workgroup (65) and several with a tail (257); S: one slot, a partial chunk of 32 (33, 50), whole chunks (512).
    Non-vacuous: for S > 1 at least a third of the expected values must lie strictly between 0 and 1 (with one slot a distance
    is 0, 1 or NaN and nothing else: there both 0 and 1 must occur)."""
    from hulk_amd.smash import panel_distances
    rng = np.random.default_rng(1000 + s)
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    inner = total = zeros = ones = 0
    for m in (1, 3, 16, 17, 33):
        for p in (1, 2, 63, 64, 65, 257):
            sm, sw = make_sketches(rng, m, s, base)
            pm, pw = make_sketches(rng, p, s, base)
            got = {}
            wants = {metric: yardsticks(sm, sw, pm, pw, metric) for metric in ("jaccard", "weightedjaccard")}
            for metric, role in VARIANTS:
                want = wants[metric][role]
                got[metric, role] = panel_distances(sm, sw, pm, pw, metric, role)
                assert_bits(got[metric, role], want, f"m {m} P {p} S {s} {metric} {role}")
                inner += int(((want > 0) & (want < 1)).sum()); total += want.size
                zeros += int((want == 0).sum()); ones += int((want == 1).sum())
            assert np.array_equal(bits(got["jaccard", "row"]), bits(got["jaccard", "column"])), "jaccard: the roles are one"
    print(f"S {s}: {inner} of {total} expected distances strictly inside (0, 1), {zeros} zeros, {ones} ones")
    if s > 1:
        assert 3 * inner >= total, "the inputs are no test: too few distances strictly between 0 and 1"
    else:
        assert zeros and ones


def test_kernel_planted_values():
    from hulk_amd.smash import panel_distances
    names = ["A", "Aneg", "B", "C", "Cr", "D", "E"]
    mins = np.array([[1, 2, 3, 4],                      # A
                     [1, 2, 3, 4],                      # Aneg: A's weights with the signs turned (equal magnitude)
                     [5, 6, 7, 8],                      # B: no slot in common with A
                     [2 ** 63 + 1, 2, 3, 4],            # C and Cr: 2^63 + 1 and 2^63 are one float64
                     [2 ** 63, 2, 3, 4],
                     [1, 2, 3, 4],                      # D: MaxFloat64 weights, the union overflows
                     [1, 2, 3, 4]], dtype=np.uint64)    # E: weights -0.0 / 0.0 only, 0 / 0
    weights = np.array([[0.5, -0.5, 0.25, -0.25],
                        [-0.5, 0.5, -0.25, 0.25],
                        [-1e-3, -2e-3, 3e-3, -4e-3],
                        [-1e-3, -2e-3, -3e-3, -4e-3],
                        [-2e-3, -2e-3, -3e-3, -4e-3],
                        [MAXF, MAXF, MAXF, MAXF],
                        [-0.0, 0.0, -0.0, 0.0]])
    ix = {n: i for i, n in enumerate(names)}
    got = {}
    for metric, role in VARIANTS:
        want = yardstick(mins, weights, mins, weights, metric, role)
        got[metric, role] = g = panel_distances(mins, weights, mins, weights, metric, role)
        print(metric, role, "\n", g)
        assert_bits(g, want, f"planted {metric} {role}")
        assert g[ix["A"], ix["A"]] == 0 and g[ix["A"], ix["Aneg"]] == 0 and g[ix["Aneg"], ix["A"]] == 0     # all slots equal
        assert g[ix["A"], ix["B"]] == 1 and g[ix["B"], ix["A"]] == 1                                         # none equal
        assert g[ix["C"], ix["Cr"]] == 0 and g[ix["Cr"], ix["C"]] == 0
    assert np.array_equal(bits(got["jaccard", "row"]), bits(got["jaccard", "column"]))
    row, col = got["weightedjaccard", "row"], got["weightedjaccard", "column"]
    assert np.isnan(row[ix["D"], ix["A"]]) and np.isnan(col[ix["A"], ix["D"]]), "Inf / Inf where the subject's weights are MaxFloat64"
    assert row[ix["D"], ix["B"]] == 1 and row[ix["A"], ix["D"]] == 0, "0 / Inf; the query's weights are never read"
    assert np.isnan(row[ix["E"]]).all() and np.isnan(col[:, ix["E"]]).all(), "0 / 0 whatever the query"
    assert got["jaccard", "row"][ix["D"], ix["E"]] == 0


def test_kernel_nan_and_inf_weights():
    """Weights that are NaN or Inf when they arrive (no sketcher writes them; a file may hold them): a NaN goes through the sums as
    it is (math.Max hands back the quiet NaN, every sum keeps it), an Inf makes the quotient Inf / Inf where a slot agrees.  The
    yardstick decides, bit for bit; sketches 0 and 1 carry NaNs of both signs, 2 and 3 infinities, 4 is plain."""
    from hulk_amd.smash import panel_distances
    rng = np.random.default_rng(77)
    s = 40
    base = rng.integers(0, 194481, size=s).astype(np.uint64)
    mins, weights = make_sketches(rng, 5, s, base)
    weights[0, 3] = np.nan; weights[1, [0, 35]] = -np.nan; weights[1, 7] = np.nan
    weights[2, 5] = np.inf; weights[3, [1, 33]] = -np.inf
    mins[:, [3, 5]] = base[[3, 5]]                               # (slots 3 and 5 agree everywhere: the special weights enter the intersection too)
    for metric, role in VARIANTS:
        want = yardstick(mins, weights, mins, weights, metric, role)
        got = panel_distances(mins, weights, mins, weights, metric, role)
        print(metric, role, "\n", got)
        assert_bits(got, want, f"NaN / Inf weights {metric} {role}")
    row = panel_distances(mins, weights, mins, weights, "weightedjaccard", "row")
    assert np.isnan(row[:3]).all() and np.isfinite(row[4]).all(), "subjects 0-2 are NaN whatever the query, the plain subject never is"
    assert np.isnan(row[3]).any() or (row[3] == 1).all()


# ---- 2. in-stream scoring ----------------------------------------------------------------------------------------------------
def interval_reads(t, I, G=20000, fresh=40, L=L):          # interval t of the stream
    from hulk_amd import synth
    genome = synth.reads_numpy(t, 1, G)[0]
    n = I if t == 0 else fresh
    starts = (np.arange(n, dtype=np.int64) * 7919) % (G - L + 1)
    rd = genome[starts[:, None] + np.arange(L)[None, :]]
    if n < I: rd = np.vstack([rd, np.full((I - n, L), ord("A"), np.uint8)])
    return np.ascontiguousarray(rd.reshape(-1)), np.arange(I + 1, dtype=np.uint64) * np.uint64(L)


@functools.lru_cache(maxsize=None)
def stream(n_reads=N_INT * I):
    """the first n_reads reads of the stream: (bases, offsets)"""
    nint = (n_reads + I - 1) // I
    bases = np.concatenate([interval_reads(t, I)[0] for t in range(nint)])[:n_reads * L]
    return bases, np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(L)


def piece(lo, hi):
    bases, _ = stream(max(hi, N_INT * I))
    return bases[lo * L:hi * L], np.arange(hi - lo + 1, dtype=np.uint64) * np.uint64(L)


def sketcher(name, **kw):
    import hulk_amd
    c = CONFIGS[name]
    kw.setdefault("snapshots", 1)
    kw.setdefault("snapshot_capacity", 64)
    return hulk_amd.GpuSketcher(K, W, c["S"], kw.pop("interval", I), c["decay"], **kw)


@functools.lru_cache(maxsize=None)
def batch_one_snapshots(name):
    g = sketcher(name, batch=1)
    g.add_reads(*stream())
    g.finish()
    _, mins, weights = g.snapshots()
    g.close()
    assert len(mins) == N_INT
    return mins, weights


def panel_from(mins, weights, seed, own=12, n_panel=N_PANEL):
    """own snapshots (spread over the trajectory), copies of them with 30 % of the slots drawn again, random sketches"""
    rng = np.random.default_rng(seed)
    S = mins.shape[1]
    pick = np.linspace(0, len(mins) - 1, own).astype(int)
    pm, pw = [mins[i].copy() for i in pick], [weights[i].copy() for i in pick]
    for i in pick:
        again = rng.random(S) < 0.3
        pm.append(np.where(again, rng.integers(0, K ** 4, size=S).astype(np.uint64), mins[i]))
        w = np.where(again, -rng.gamma(2.0, 1e-3, size=S), weights[i])
        pw.append(np.where(np.isfinite(w) & (np.abs(w) < 1e300), w, -1e-3))
    n_random = n_panel - len(pm)
    pm += list(rng.integers(0, K ** 4, size=(n_random, S)).astype(np.uint64))
    pw += list(-rng.gamma(2.0, 1e-3, size=(n_random, S)))
    return np.stack(pm), np.stack(pw)


@functools.lru_cache(maxsize=None)
def panel(name):
    return panel_from(*batch_one_snapshots(name), seed=len(name))


def scored_run(name, metric, role, pm=None, pw=None, feed=None, **kw):
    """one context with the panel: (info, mins, weights, distances) of everything the ring holds"""
    if pm is None:
        pm, pw = panel(name)
    g = sketcher(name, **kw)
    g.set_panel(pm, pw, metric, role)
    if feed is None:
        g.add_reads(*stream())
    else:
        feed(g)
    g.finish()
    first = g.snapshot_count()[1]
    info, mins, weights = g.snapshots(first)
    dist = g.snapshot_distances(first)
    g.close()
    return info, mins, weights, dist


@functools.lru_cache(maxsize=None)
def reference_run(name, metric, role):
    return scored_run(name, metric, role, batch=1, work_lanes=1)[3]


@pytest.mark.parametrize("name", ["nodrift", "decay"])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("batch", [1, 3, 16])
def test_in_stream_scoring(name, lanes, batch):
    pm, pw = panel(name)
    assert pm.shape == (N_PANEL, CONFIGS[name]["S"])
    for metric, role in VARIANTS[1:]:                               # (jaccard row == jaccard column is the kernel test's)
        info, mins, weights, dist = scored_run(name, metric, role, batch=batch, work_lanes=lanes)
        assert [x["ordinal"] for x in info] == list(range(1, N_INT + 1)) and dist.shape == (N_INT, N_PANEL)
        want = yardstick(mins, weights, pm, pw, metric, role)
        moves = sum(1 for t in range(1, N_INT) if not np.array_equal(bits(want[t]), bits(want[t - 1])))
        inner = int(((want > 0) & (want < 1)).sum())
        print(f"{name} {metric} {role}: {moves} of {N_INT - 1} transitions move the distance row, {inner} of {want.size} values inside (0, 1)")
        assert moves >= CONFIGS[name]["min_moves"] and inner >= want.size // 8, "the trajectory of distances does not move: no test"
        assert_bits(dist, want, f"{name} batch {batch} lanes {lanes} {metric} {role}")
        assert_bits(dist, reference_run(name, metric, role), f"{name} batch {batch} lanes {lanes} {metric} {role} against batch 1")


# ---- 3. paths that are easy to forget ----------------------------------------------------------------------------------------
def test_batches_the_flush_skips_are_scored():
    """the construction of test_batches_the_flush_skips_still_record (tests/test_gpu_snapshots.py): uniform reads, no drift,
    three batches of 16; the last one must not visit a tile (k_flush_decide passes it over, k_cws_apply_snap copies the sketch
    as it stands) and its snapshots are scored all the same"""
    import hulk_amd
    from hulk_amd import synth
    S, I2, T, batches = 64, 2000, 16, 3
    n = T * I2

    def run(pm=None, pw=None):
        g = hulk_amd.GpuSketcher(K, W, S, I2, 1.0, batch=T, snapshots=1, snapshot_capacity=T * batches)
        if pm is not None:
            g.set_panel(pm, pw, "weightedjaccard", "row")
        for b in range(batches - 1):
            g.add_reads(*synth.reads_numpy(b * n, n, L))
        before, _ = g.scan_stats()
        g.add_reads(*synth.reads_numpy((batches - 1) * n, n, L))
        after, _ = g.scan_stats()
        assert after == before, "the last batch still visited tiles: this run says nothing about skipped ones"
        g.finish()
        _, mins, weights = g.snapshots()
        dist = g.snapshot_distances() if pm is not None else None
        g.close()
        return mins, weights, dist
    mins0, weights0, _ = run()
    pm, pw = panel_from(mins0, weights0, seed=5, own=4)
    mins, weights, dist = run(pm, pw)
    assert np.array_equal(mins, mins0) and np.array_equal(bits(weights), bits(weights0))
    want = yardstick(mins, weights, pm, pw, "weightedjaccard", "row")
    assert (want[-1] == 0).any() and ((want[-1] > 0) & (want[-1] < 1)).any()
    assert_bits(dist, want, "skipped batches")
    assert np.array_equal(bits(dist[-T:]), np.tile(bits(dist[-1]), (T, 1)))


@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_half_an_interval_at_the_end(name):
    pm, pw = panel(name)
    n = N_INT * I + I // 2
    info, mins, weights, dist = scored_run(name, "weightedjaccard", "column", feed=lambda g: g.add_reads(*stream(n)))
    assert len(info) == N_INT + 1 and info[-1] == {"ordinal": N_INT + 1, "n_reads": n}
    assert_bits(dist, yardstick(mins, weights, pm, pw, "weightedjaccard", "column"), name)
    assert_bits(dist[:N_INT], reference_run(name, "weightedjaccard", "column"), name)


def test_every_third():
    pm, pw = panel("nodrift")
    info, mins, weights, dist = scored_run("nodrift", "weightedjaccard", "row", snapshots=3)
    assert [x["ordinal"] for x in info] == list(range(3, N_INT + 1, 3)) + [N_INT]
    assert_bits(dist, yardstick(mins, weights, pm, pw, "weightedjaccard", "row"), "every = 3")
    idx = [o - 1 for o in range(3, N_INT + 1, 3)] + [N_INT - 1]
    assert_bits(dist, reference_run("nodrift", "weightedjaccard", "row")[idx], "every = 3 against every = 1")


@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_ring_of_four_with_the_scored_callback_loses_nothing(name):
    """capacity 4 bounds a flush to 4 intervals; the first call holds 2, so every later flush takes entries 2, 3, 0, 1: the
    ring wraps inside one flush"""
    pm, pw = panel(name)
    got = []
    g = sketcher(name, snapshot_capacity=4, batch=16)
    g.set_panel(pm, pw, "weightedjaccard", "row")
    g.on_snapshot_scored(lambda info, m, w, d: got.append((info, m, w, d)) and None)
    assert g.batch_size == 4
    g.add_reads(*piece(0, 2 * I))
    g.add_reads(*piece(2 * I, N_INT * I))
    g.finish()
    g.close()
    assert [x[0]["ordinal"] for x in got] == list(range(1, N_INT + 1))
    mins, weights, dist = (np.stack([x[i] for x in got]) for i in (1, 2, 3))
    bm, bw = batch_one_snapshots(name)
    assert np.array_equal(mins, bm) and np.array_equal(bits(weights), bits(bw))
    assert_bits(dist, yardstick(mins, weights, pm, pw, "weightedjaccard", "row"), name)
    assert_bits(dist, reference_run(name, "weightedjaccard", "row"), name)


def test_ring_of_four_without_a_callback_drops_the_oldest():
    from hulk_amd import HulkError
    pm, pw = panel("nodrift")
    g = sketcher("nodrift", snapshot_capacity=4)
    g.set_panel(pm, pw, "jaccard", "row")
    g.add_reads(*piece(0, 2 * I))
    g.add_reads(*piece(2 * I, N_INT * I))
    g.finish()
    assert g.snapshot_count() == (N_INT, N_INT - 4)
    _, mins, weights = g.snapshots(N_INT - 4)
    dist = g.snapshot_distances(N_INT - 4)
    assert_bits(dist, yardstick(mins, weights, pm, pw, "jaccard", "row"), "ring of 4")
    assert_bits(dist, reference_run("nodrift", "jaccard", "column")[N_INT - 4:], "ring of 4")
    for first, n in ((N_INT - 5, 2), (N_INT - 1, 2)):
        with pytest.raises(HulkError) as e1:
            g.snapshots(first, n)
        with pytest.raises(HulkError) as e2:
            g.snapshot_distances(first, n)
        assert e1.value.code == e2.value.code == -30 and e1.value.message == e2.value.message
    g.close()


@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_slot_shard(name):
    """A slot-shard context leaves the slots it does not own at 0 / MaxFloat64.  The panel here has finite weights and, in its
    first half, the shard's own mins (0 in the unowned slots): with the snapshot as the subject the union and the intersection
    both overflow (NaN), with the panel sketch as the subject everything is finite."""
    S = CONFIGS[name]["S"]
    q = S // 4
    fm, fw = batch_one_snapshots(name)
    pm, pw = panel_from(fm, fw, seed=11)
    other = np.r_[0:q, 2 * q:S]
    pm[:N_PANEL // 2, other] = 0
    for metric, role in (("weightedjaccard", "row"), ("weightedjaccard", "column"), ("jaccard", "row")):
        info, mins, weights, dist = scored_run(name, metric, role, pm, pw, slot_begin=q, slot_count=q)
        assert (mins[:, other] == 0).all() and (weights[:, other] == MAXF).all() and len(info) == N_INT
        assert_bits(dist, yardstick(mins, weights, pm, pw, metric, role), f"{name} shard {metric} {role}")
        if metric == "weightedjaccard" and role == "row":
            assert np.isnan(dist[:, :N_PANEL // 2]).all() and (dist[:, N_PANEL // 2:] == 1).any()
        else:
            assert np.isfinite(dist).all() and ((dist > 0) & (dist < 1)).any()


# ---- 4. state errors ---------------------------------------------------------------------------------------------------------
def test_state_errors():
    import hulk_amd
    from hulk_amd import HulkError, _lib
    STATE, ARG = -34, -30
    S = CONFIGS["nodrift"]["S"]
    pm, pw = panel("nodrift")
    g = hulk_amd.GpuSketcher(K, W, S, I)
    for call in (lambda: g.set_panel(pm, pw), g.snapshot_distances, lambda: g.on_snapshot_scored(lambda *a: None)):
        with pytest.raises(HulkError) as e:                         # before hulk_set_snapshots
            call()
        assert e.value.code == STATE
    g.close()
    g = sketcher("nodrift")
    with pytest.raises(HulkError) as e:                             # the getter without a panel
        g.snapshot_distances()
    assert e.value.code == STATE and "panel" in e.value.message
    with pytest.raises(HulkError) as e:
        g.set_panel(pm[:, :S - 1], pw[:, :S - 1])
    assert e.value.code == ARG and e.value.message.endswith(f"sketch length mismatch: {S} vs {S - 1}\n")
    L_ = g._L
    assert L_.hulk_set_panel(g._ctx, pm.ctypes.data, pw.ctypes.data, _lib.HULK_PANEL_MAX + 1, S, 0, 0) == ARG      # (refused before it is read)
    assert b"at most 65536" in L_.hulk_last_error(g._ctx)
    assert L_.hulk_set_panel(g._ctx, pm.ctypes.data, pw.ctypes.data, N_PANEL, S, 2, 0) == ARG          # metric
    assert L_.hulk_set_panel(g._ctx, pm.ctypes.data, pw.ctypes.data, N_PANEL, S, 0, 2) == ARG          # role
    assert L_.hulk_set_panel(g._ctx, None, pw.ctypes.data, N_PANEL, S, 0, 0) == ARG
    g.set_panel(pm, pw)
    assert g.snapshot_distances().shape == (0, N_PANEL)
    assert L_.hulk_set_panel(g._ctx, None, None, 0, S, 0, 0) == 0   # n_panel == 0 removes it
    with pytest.raises(HulkError) as e:
        g.snapshot_distances()
    assert e.value.code == STATE
    g.set_panel(pm, pw)
    assert L_.hulk_set_snapshots(g._ctx, 1, 64) == 0                # ... and so does setting the snapshots again
    with pytest.raises(HulkError) as e:
        g.snapshot_distances()
    assert e.value.code == STATE
    g.add_reads(*piece(0, 10))
    for call in (lambda: g.set_panel(pm, pw), lambda: g.on_snapshot_scored(lambda *a: None)):
        with pytest.raises(HulkError) as e:                         # after the first read
            call()
        assert e.value.code == STATE
    g.add_reads(*piece(10, 2 * I))
    g.finish()
    assert g.snapshot_count() == (2, 0)                             # the context is still good for what it is for
    g.close()


def test_scored_callback_failure_ends_the_run():
    from hulk_amd import HulkError
    pm, pw = panel("nodrift")
    calls = []

    def boom(info, m, w, d):
        calls.append((info["ordinal"], d.shape))
        if len(calls) == 3:
            raise RuntimeError("stop here")
    g = sketcher("nodrift")
    g.set_panel(pm, pw)
    g.on_snapshot(lambda *a: calls.append("the three-argument callable was replaced"))
    g.on_snapshot_scored(boom)
    with pytest.raises(HulkError, match="snapshot callback failed") as e:
        g.add_reads(*stream())
        g.finish()
    assert e.value.code == -34 and isinstance(e.value.__cause__, RuntimeError)
    assert calls == [(1, (N_PANEL,)), (2, (N_PANEL,)), (3, (N_PANEL,))]
    with pytest.raises(HulkError, match="snapshot callback failed"):
        g.finish()
    g.close()


# ---- 5. no panel means no change ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_no_panel_means_no_change(name):
    from hulk_amd import _lib
    pm, pw = panel(name)
    out = {}
    for with_panel in (False, True):
        g = sketcher(name, flags=_lib.HULK_FLAG_NO_OVERLAP)
        if with_panel:
            g.set_panel(pm, pw, "weightedjaccard", "row")
        g.set_profiling(32)
        g.add_reads(*stream())
        g.finish()
        table = g.profile_table()
        _, mins, weights = g.snapshots()
        g.close()
        out[with_panel] = (table, mins, weights)
    assert np.array_equal(out[False][1], out[True][1]) and np.array_equal(bits(out[False][2]), bits(out[True][2]))
    bm, bw = batch_one_snapshots(name)
    assert np.array_equal(out[False][1], bm) and np.array_equal(bits(out[False][2]), bits(bw))
    assert "k_snap_panel" not in out[False][0] and out[False][0], sorted(out[False][0])
    assert out[True][0]["k_snap_panel"][0] >= 3, out[True][0].get("k_snap_panel")
    others = {k: v[0] for k, v in out[True][0].items() if k != "k_snap_panel"}
    assert others == {k: v[0] for k, v in out[False][0].items()}, "the panel changed what else is launched"
    # a scored callback on a context without a panel: the three-argument delivery with an empty array
    got = []
    g = sketcher(name)
    g.on_snapshot_scored(lambda info, m, w, d: got.append((m, w, d)) and None)
    g.add_reads(*stream())
    g.finish()
    g.close()
    assert len(got) == N_INT and all(x[2].shape == (0,) for x in got)
    assert np.array_equal(np.stack([x[0] for x in got]), bm) and np.array_equal(bits(np.stack([x[1] for x in got])), bits(bw))


# ---- 6. the CLI --------------------------------------------------------------------------------------------------------------
def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "hulk_amd"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)


def write_fastq(path, lo, hi):
    rows = piece(lo, hi)[0].reshape(-1, L)
    qual = b"I" * L
    with open(path, "wb") as fh:
        for i, r in enumerate(rows):
            fh.write(b"@r%d\n" % i + r.tobytes() + b"\n+\n" + qual + b"\n")


def test_cli_panel_end_to_end(tmp_path):
    S = 64
    base = ["sketch", "-k", str(K), "-w", str(W), "-s", str(S)]
    os.makedirs(tmp_path / "panel")
    # three panel sketches: prefixes of the stream the fourth input continues, so that they share slots with its snapshots
    for j, hi in enumerate((2 * I, 7 * I, 12 * I)):
        write_fastq(str(tmp_path / f"p{j}.fq"), 0, hi)
        r = run_cli(base + ["-f", str(tmp_path / f"p{j}.fq"), "-i", str(I), "-o", str(tmp_path / "panel" / f"ref{j}")], str(tmp_path))
        assert r.returncode == 0, r.stdout + r.stderr
    write_fastq(str(tmp_path / "run.fq"), 0, 16 * I)
    r = run_cli(base + ["-f", str(tmp_path / "run.fq"), "-i", str(I), "-o", "run", "--streamEvery", "2", "--panel", str(tmp_path / "panel"),
                        "--panelMetric", "weightedjaccard"], str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(tmp_path / "run.trajectory.csv").read().splitlines()
    refs = [str(tmp_path / "panel" / f"ref{j}.json") for j in range(3)]
    assert lines[0] == "ordinal,reads," + ",".join(refs)
    rows = [x.split(",") for x in lines[1:]]
    assert [(int(x[0]), int(x[1])) for x in rows] == [(o, o * I) for o in range(2, 17, 2)]
    assert len({tuple(x[2:]) for x in rows}) >= 3, "the trajectory does not move"
    for row in (rows[1], rows[-1]):
        ordinal = int(row[0])
        d = tmp_path / f"with{ordinal}"
        shutil.copytree(tmp_path / "panel", d)
        name = "%08d.json" % ordinal
        shutil.copy(tmp_path / "run.snapshots" / name, d / name)     # sorts in front of ref*.json
        rs = run_cli(["smash", "-k", str(K), "-d", str(d), "-m", "weightedjaccard", "-o", f"m{ordinal}"], str(tmp_path))
        assert rs.returncode == 0, rs.stdout + rs.stderr
        m = [x.split(",") for x in open(tmp_path / f"m{ordinal}.hulk-matrix.csv").read().splitlines()]
        at = m[0].index(str(d / name))
        mine = m[1 + at]
        assert row[2:] == mine[:at] + mine[at + 1:], f"snapshot {ordinal}: the trajectory line is not smash's row"
    last = [float(x) for x in rows[-1][2:]]
    best = max(range(3), key=lambda j: (last[j] == last[j], last[j], -j))
    final = [x for x in r.stdout.splitlines() if "closest panel sketch" in x]
    assert len(final) == 1 and final[0].endswith(f"closest panel sketch to snapshot 16: {refs[best]} ({rows[-1][2 + best]})"), final
    assert last[2] > last[0], "the longest prefix of the stream is closer to its end than the shortest"


# ---- 7. the C++ host ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_cpp_host_matches_the_python_binding(name, tmp_path):
    """hulk::Boss::SetPanel / Snapshot::Distances (include/hulk.hpp) against GpuSketcher.snapshot_distances(), via %a"""
    c = CONFIGS[name]
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    exe = str(tmp_path / "panel_driver")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "panel_driver.cpp"), "-o", exe,
                        "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    pm, pw = panel(name)
    bases, _ = stream()
    txt, ptxt = tmp_path / "reads.txt", tmp_path / "panel.txt"
    txt.write_bytes(b"\n".join(r.tobytes() for r in bases.reshape(-1, L)) + b"\n")
    ptxt.write_text("".join(" ".join([str(int(v)) for v in m] + [float(v).hex() for v in w]) + "\n" for m, w in zip(pm, pw)))
    for metric, role in (("weightedjaccard", "row"), ("weightedjaccard", "column")):
        want = reference_run(name, metric, role)
        for mode, cap in (("collect", "64"), ("callback", "4")):
            args = [str(txt), str(ptxt), str(K), str(W), str(c["S"]), str(I), repr(c["decay"]), "1", cap, metric, role]
            p = subprocess.run([exe, mode] + args, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
            out = p.stdout.splitlines()
            assert out[-1] == f"final {N_INT if mode == 'callback' else 0}"
            rows = [x.split() for x in out[:-1]]
            assert [(int(x[0]), int(x[1])) for x in rows] == [(o, o * I) for o in range(1, N_INT + 1)], mode
            got = np.array([[float.fromhex(v) if "nan" not in v else float("nan") for v in x[2:]] for x in rows])
            assert not np.isnan(want).any()
            assert_bits(got, want, f"{name} {mode} {metric} {role}")
        # a Boss that was moved after SetPanel still knows its panel; EnableSnapshots behind SetPanel drops it on both sides
        args = [str(txt), str(ptxt), str(K), str(W), str(c["S"]), str(I), repr(c["decay"]), "1", "64", metric, role]
        p = subprocess.run([exe, "moved"] + args, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        rows = [x.split() for x in p.stdout.splitlines()[:-1]]
        assert len(rows) == N_INT and all(len(x) == 2 + N_PANEL for x in rows), "a moved Boss lost its panel"
        assert_bits(np.array([[float.fromhex(v) for v in x[2:]] for x in rows]), want, f"{name} moved {metric} {role}")
    p = subprocess.run([exe, "reenable"] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [x.split() for x in p.stdout.splitlines()[:-1]]
    assert [(int(x[0]), int(x[1])) for x in rows] == [(o, o * I) for o in range(1, N_INT + 1)] and all(len(x) == 2 for x in rows)
