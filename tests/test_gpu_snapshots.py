"""Sketch snapshots (hulk_set_snapshots ...): the histosketch after every flushed spectrum, recorded inside the batched flush.

Ground truth:
  (a) the oracle, unchanged: pyorc.Sketcher(..., interval=I), fed exactly I reads, .sketch() read, repeated — mins equal,
      weights within the project's standing tolerances (1e-9 relative, 1e-7 with decay);
  (b) bit for bit, the library itself without the feature: a second context without snapshots, batch = 1, fed one interval
      at a time with hulk_get_sketch after each.

The input has to make the sketch MOVE: with the uniform reads of hulk_amd/synth.py and no drift the sketch is final after the
first interval, and an implementation that copied the final sketch into every snapshot would pass.  interval_reads() cuts the
reads of every interval from a fresh synthetic genome, with homopolymer filler so that the count-min counters stay low; the
trajectory tests assert on the oracle's own trajectory that it moves before they compare anything."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import pyorc

pytestmark = pytest.mark.gpu

K, W, I, N_INT, L = 15, 9, 400, 40, 150
MAXF = 1.7976931348623157e308
CONFIGS = {"nodrift": dict(S=256, decay=1.0, rtol=1e-9, min_moves=8, window=15),
           "decay": dict(S=64, decay=0.02, rtol=1e-7, min_moves=30, window=39)}


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


@functools.lru_cache(maxsize=None)
def oracle_trajectory(name):
    """(a): mins[N_INT][S], weights[N_INT][S] — the oracle fed one interval at a time"""
    c = CONFIGS[name]
    o = pyorc.Sketcher(K, W, c["S"], 0, c["decay"], I)
    mins, weights = [], []
    for t in range(N_INT):
        o.add_reads(*piece(t * I, (t + 1) * I))
        m, w = o.sketch()
        mins.append(np.array(m, dtype=np.uint64)); weights.append(np.array(w, dtype=np.float64))
    o.close()
    return np.stack(mins), np.stack(weights)


@functools.lru_cache(maxsize=None)
def library_trajectory(name):
    """(b): the library without the feature, batch = 1, hulk_get_sketch after every interval"""
    import hulk_amd
    c = CONFIGS[name]
    g = hulk_amd.GpuSketcher(K, W, c["S"], I, c["decay"], batch=1)
    mins, weights = [], []
    for t in range(N_INT):
        g.add_reads(*piece(t * I, (t + 1) * I))
        m, w = g.sketch()
        mins.append(m); weights.append(w)
    g.finish()
    fm, fw = g.sketch()
    g.close()
    assert np.array_equal(fm, mins[-1]) and np.array_equal(fw, weights[-1])
    return np.stack(mins), np.stack(weights)


def sketcher(name, **kw):
    import hulk_amd
    c = CONFIGS[name]
    kw.setdefault("snapshots", 1)
    kw.setdefault("snapshot_capacity", 64)
    return hulk_amd.GpuSketcher(K, W, c["S"], kw.pop("interval", I), c["decay"], **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_bitwise(mins, weights, want_m, want_w, what=""):
    assert mins.shape == want_m.shape, what
    assert np.array_equal(mins, want_m), f"{what}: mins differ in snapshots {sorted(set(np.nonzero(mins != want_m)[0].tolist()))}"
    assert np.array_equal(bits(weights), bits(want_w)), f"{what}: weights differ in snapshots {sorted(set(np.nonzero(bits(weights) != bits(want_w))[0].tolist()))}"


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_every_snapshot_against_the_oracle(name):
    c = CONFIGS[name]
    om, ow = oracle_trajectory(name)
    moved = [(om[t] != om[t - 1]).sum() for t in range(1, N_INT)]
    print(f"{name}: slots whose min moved per transition: {moved}")
    assert sum(1 for x in moved[:c["window"]] if x) >= c["min_moves"], "the oracle's trajectory does not move: the input is no test"
    g = sketcher(name, batch=16)
    g.add_reads(*stream())
    g.finish()
    info, mins, weights = g.snapshots()
    assert [i["ordinal"] for i in info] == list(range(1, N_INT + 1))
    assert [i["n_reads"] for i in info] == [I * o for o in range(1, N_INT + 1)]
    assert g.snapshot_count() == (N_INT, 0)
    worst = 0.0
    for t in range(N_INT):
        assert np.array_equal(mins[t], om[t]), f"snapshot {t}: {int((mins[t] != om[t]).sum())} mins differ from the oracle"
        worst = max(worst, float(np.max(np.abs(weights[t] - ow[t]) / np.abs(ow[t]))))
        assert np.allclose(weights[t], ow[t], rtol=c["rtol"], atol=0), f"snapshot {t}: weights differ from the oracle"
    print(f"{name}: largest relative weight error against the oracle {worst:.3e}")
    fm, fw = g.sketch()
    assert np.array_equal(mins[-1], fm) and np.array_equal(bits(weights[-1]), bits(fw)), "last snapshot != hulk_get_sketch"
    g.close()
    import hulk_amd
    plain = hulk_amd.GpuSketcher(K, W, c["S"], I, c["decay"], batch=16)
    plain.add_reads(*stream())
    plain.finish()
    pm, pw = plain.sketch()
    plain.close()
    assert np.array_equal(pm, fm) and np.array_equal(bits(pw), bits(fw)), "snapshots changed the final sketch"


# ---- 2. bit for bit against the library without the feature ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nodrift", "decay"])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("batch", [1, 3, 16])
def test_bitwise_against_batch_one(name, lanes, batch):
    lm, lw = library_trajectory(name)
    assert sum(1 for t in range(1, N_INT) if (lm[t] != lm[t - 1]).any()) >= CONFIGS[name]["min_moves"]
    g = sketcher(name, batch=batch, work_lanes=lanes)
    assert g.batch_size == batch
    g.add_reads(*stream())
    g.finish()
    _, mins, weights = g.snapshots()
    g.close()
    assert_bitwise(mins, weights, lm, lw, f"{name} batch {batch} lanes {lanes}")


@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_calls_that_do_not_line_up_with_intervals(name):
    lm, lw = library_trajectory(name)
    g = sketcher(name)
    sizes, at, n = [37, 1000, 5, 3999, 1, 400, 2763, 6400], 0, N_INT * I
    i = 0
    while at < n:
        step = min(sizes[i % len(sizes)], n - at)
        g.add_reads(*piece(at, at + step))
        at += step; i += 1
    g.finish()
    info, mins, weights = g.snapshots()
    g.close()
    assert [x["n_reads"] for x in info] == [I * o for o in range(1, N_INT + 1)]
    assert_bitwise(mins, weights, lm, lw, name)


def write_fastq(path):
    bases, _ = stream()
    rows = bases.reshape(-1, L)
    qual = b"I" * L
    with open(path, "wb") as fh:
        for i, r in enumerate(rows):
            fh.write(b"@r%d\n" % i + r.tobytes() + b"\n+\n" + qual + b"\n")


@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_through_sketch_files(name, tmp_path):
    lm, lw = library_trajectory(name)
    fq = str(tmp_path / "stream.fq")
    write_fastq(fq)
    g = sketcher(name)
    st = g.sketch_files([fq])
    assert st["n_seqs"] == N_INT * I
    g.finish()
    info, mins, weights = g.snapshots()
    g.close()
    assert [x["ordinal"] for x in info] == list(range(1, N_INT + 1))
    assert_bitwise(mins, weights, lm, lw, name)


# ---- 3. which spectra are recorded -------------------------------------------------------------------------------------------
def test_every_third_and_the_end_of_the_stream():
    lm, lw = library_trajectory("nodrift")
    g = sketcher("nodrift", snapshots=3)
    g.add_reads(*stream())
    g.finish()
    info, mins, weights = g.snapshots()
    g.close()
    # 3, 6, ... 39, and the EOF flush: reads arrived since snapshot 39, its (empty) spectrum takes no new ordinal
    assert [x["ordinal"] for x in info] == list(range(3, N_INT + 1, 3)) + [N_INT]
    assert [x["n_reads"] for x in info] == [I * o for o in range(3, N_INT + 1, 3)] + [I * N_INT]
    idx = [o - 1 for o in range(3, N_INT + 1, 3)] + [N_INT - 1]
    assert_bitwise(mins, weights, lm[idx], lw[idx], "every = 3")


@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_half_an_interval_at_the_end(name):
    lm, lw = library_trajectory(name)
    n = N_INT * I + I // 2
    g = sketcher(name)
    g.add_reads(*stream(n))
    g.finish()
    info, mins, weights = g.snapshots()
    fm, fw = g.sketch()
    g.close()
    assert len(info) == N_INT + 1 and info[-1] == {"ordinal": N_INT + 1, "n_reads": 16200}
    assert_bitwise(mins[:N_INT], weights[:N_INT], lm, lw, name)
    assert np.array_equal(mins[-1], fm) and np.array_equal(bits(weights[-1]), bits(fw))
    o = pyorc.Sketcher(K, W, CONFIGS[name]["S"], 0, CONFIGS[name]["decay"], I)
    o.add_reads(*stream(n)); o.finish()
    om, ow = o.sketch(); o.close()
    assert np.array_equal(fm, om) and np.allclose(fw, ow, rtol=CONFIGS[name]["rtol"], atol=0)


def test_a_stream_of_whole_intervals_gets_no_duplicate():
    g = sketcher("nodrift")
    g.add_reads(*stream())
    assert g.snapshot_count()[0] == N_INT
    g.finish()
    assert g.snapshot_count() == (N_INT, 0)
    g.close()


def test_explicit_flushes_without_an_interval():
    import hulk_amd
    S = CONFIGS["nodrift"]["S"]
    g = sketcher("nodrift", interval=0)
    ref = hulk_amd.GpuSketcher(K, W, S, 0, 1.0)
    want_m, want_w = [], []
    for t in range(5):
        for x in (g, ref):
            x.add_reads(*piece(t * I, (t + 1) * I)); x.flush()
        m, w = ref.sketch()
        want_m.append(m); want_w.append(w)
    assert g.snapshot_count() == (5, 0)
    g.finish(); ref.finish()
    info, mins, weights = g.snapshots()
    g.close(); ref.close()
    assert info == [{"ordinal": o, "n_reads": I * o} for o in range(1, 6)]          # (nothing arrived behind the last flush)
    assert_bitwise(mins, weights, np.stack(want_m), np.stack(want_w), "explicit flushes")
    assert any((mins[t] != mins[t - 1]).any() for t in range(1, 5))


# ---- 4. the steady state: batches k_flush_decide passes over -----------------------------------------------------------------
def test_batches_the_flush_skips_still_record():
    """Uniform synth reads, no drift: after the first batch no element can lower any weight, k_flush_decide raises skip_exact
    and the scan, the resolve and the candidates are not run — the ring entries of such a batch must be written all the same.
    Measured on the MI355X (k = 15, S = 64, I = 2000, batch 16): the first batch visits 1584 of its 1600 tiles, every later
    one none (tiles_visited stays at 1584 from interval 17 on); the test feeds three batches and fails if the last one still
    visited a tile, so it cannot pass without exercising the skipped path."""
    import hulk_amd
    from hulk_amd import synth
    S, I2, T, batches = 64, 2000, 16, 3
    g = hulk_amd.GpuSketcher(K, W, S, I2, 1.0, batch=T, snapshots=1, snapshot_capacity=T * batches)
    n = T * I2
    for b in range(batches - 1):
        g.add_reads(*synth.reads_numpy(b * n, n, L))
    before, _ = g.scan_stats()
    sm, sw = g.sketch()
    g.add_reads(*synth.reads_numpy((batches - 1) * n, n, L))
    after, _ = g.scan_stats()
    print(f"tiles visited before the last batch {before}, after {after}")
    assert after == before, "the last batch still visited tiles: feed more batches, this run says nothing about skipped ones"
    g.finish()
    info, mins, weights = g.snapshots()
    fm, fw = g.sketch()
    g.close()
    assert [x["ordinal"] for x in info] == list(range(1, T * batches + 1))
    assert np.array_equal(fm, sm) and np.array_equal(bits(fw), bits(sw))
    for t in range(T * (batches - 1), T * batches):
        assert np.array_equal(mins[t], fm) and np.array_equal(bits(weights[t]), bits(fw)), f"snapshot {t} of the skipped batch"
    o = pyorc.Sketcher(K, W, S, 0, 1.0, I2)
    o.add_reads(*synth.reads_numpy(0, I2, L))
    om, ow = o.sketch(); o.close()
    assert np.array_equal(mins[0], om) and np.allclose(weights[0], ow, rtol=1e-9, atol=0)


# ---- 5. a slot shard ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_slot_shard(name):
    lm, lw = library_trajectory(name)
    S = CONFIGS[name]["S"]
    q = S // 4
    g = sketcher(name, slot_begin=q, slot_count=q)
    g.add_reads(*stream())
    g.finish()
    _, mins, weights = g.snapshots()
    g.close()
    assert_bitwise(mins[:, q:2 * q], weights[:, q:2 * q], lm[:, q:2 * q], lw[:, q:2 * q], name)
    other = np.r_[0:q, 2 * q:S]
    assert (mins[:, other] == 0).all() and (weights[:, other] == MAXF).all()


# ---- 6. the ring -------------------------------------------------------------------------------------------------------------
def test_ring_drops_the_oldest_without_a_callback():
    from hulk_amd import HulkError
    lm, lw = library_trajectory("nodrift")
    g = sketcher("nodrift", snapshot_capacity=8)
    g.add_reads(*stream())
    g.finish()
    assert g.snapshot_count() == (N_INT, N_INT - 8)
    info, mins, weights = g.snapshots(first=N_INT - 8)
    assert [x["ordinal"] for x in info] == list(range(N_INT - 7, N_INT + 1))
    assert_bitwise(mins, weights, lm[N_INT - 8:], lw[N_INT - 8:], "ring of 8")
    with pytest.raises(HulkError) as e:
        g.snapshots(first=N_INT - 9, n=2)
    assert e.value.code == -30
    with pytest.raises(HulkError) as e:
        g.snapshots(first=N_INT - 1, n=2)
    assert e.value.code == -30
    g.close()


@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_ring_of_four_with_a_callback_loses_nothing(name):
    lm, lw = library_trajectory(name)
    got = []
    g = sketcher(name, snapshot_capacity=4, batch=16)
    g.on_snapshot(lambda info, m, w: got.append((info, m, w)) and None)
    g.add_reads(*stream())
    g.finish()
    g.close()
    assert [x[0]["ordinal"] for x in got] == list(range(1, N_INT + 1))
    assert_bitwise(np.stack([x[1] for x in got]), np.stack([x[2] for x in got]), lm, lw, name)


# ---- 7. the callback ---------------------------------------------------------------------------------------------------------
def test_callback_delivery_poll_and_finish():
    got = []
    g = sketcher("nodrift")
    twin = sketcher("nodrift")
    g.on_snapshot(lambda info, m, w: got.append((info, m, w)) and None)
    half = 20 * I + 57
    g.add_reads(*piece(0, half)); twin.add_reads(*piece(0, half))
    g.synchronize()
    n0 = len(got)
    n1 = g.poll_snapshots()
    assert n0 + n1 == len(got) == g.snapshot_count()[0] == 20, "after hulk_synchronize a poll delivers everything recorded"
    assert g.poll_snapshots() == 0
    g.add_reads(*piece(half, N_INT * I)); twin.add_reads(*piece(half, N_INT * I))
    g.finish(); twin.finish()
    assert len(got) == N_INT and g.poll_snapshots() == 0
    info, mins, weights = twin.snapshots()
    assert [x[0] for x in got] == info
    assert_bitwise(np.stack([x[1] for x in got]), np.stack([x[2] for x in got]), mins, weights, "callback against hulk_get_snapshots")
    gi, gm, gw = g.snapshots()                                     # (the ring is still readable on a context with a callback)
    assert gi == info and np.array_equal(gm, mins)
    g.close(); twin.close()


def test_callback_failure_ends_the_run():
    from hulk_amd import HulkError
    calls = []

    def boom(info, m, w):
        calls.append(info["ordinal"])
        if len(calls) == 3:
            raise RuntimeError("stop here")
    g = sketcher("nodrift")
    g.on_snapshot(boom)
    with pytest.raises(HulkError, match="snapshot callback failed") as e:
        g.add_reads(*stream())
        g.finish()
    assert e.value.code == -34 and isinstance(e.value.__cause__, RuntimeError)
    assert calls == [1, 2, 3]
    with pytest.raises(HulkError, match="snapshot callback failed"):
        g.add_reads(*piece(0, 10))
    with pytest.raises(HulkError, match="snapshot callback failed"):
        g.finish()
    g.close()


# ---- 8. state errors ---------------------------------------------------------------------------------------------------------
def test_state_errors():
    import ctypes
    import hulk_amd
    from hulk_amd import HulkError, _lib
    STATE = -34                                                     # HULK_ERR_STATE
    S = CONFIGS["nodrift"]["S"]
    g = hulk_amd.GpuSketcher(K, W, S, I)
    for call in (g.snapshot_count, g.snapshots, g.poll_snapshots, lambda: g.on_snapshot(lambda *a: None)):
        with pytest.raises(HulkError) as e:
            call()
        assert e.value.code == STATE
    L_ = g._L
    assert L_.hulk_set_snapshots(g._ctx, 0, 0) == 0                 # every = 0: off
    with pytest.raises(HulkError):
        g.snapshot_count()
    assert L_.hulk_set_snapshots(g._ctx, 2, 0) == 0 and g.snapshot_count() == (0, 0)
    assert L_.hulk_set_snapshots(g._ctx, 0, 0) == 0                 # ... and off again
    g.add_reads(*piece(0, 10))
    assert L_.hulk_set_snapshots(g._ctx, 1, 0) == STATE, "hulk_set_snapshots after the first read"
    g.close()
    g = sketcher("nodrift")
    g.add_reads(*piece(0, 10))
    with pytest.raises(HulkError) as e:
        g.on_snapshot(lambda *a: None)
    assert e.value.code == STATE
    g.close()
    g = sketcher("nodrift")
    null = ctypes.c_void_p(0)
    refused = {
        "hulk_bin_reads_device": lambda: L_.hulk_bin_reads_device(g._ctx, null, null, 0, 0, 0, 0),
        "hulk_bin_reads_device_at": lambda: L_.hulk_bin_reads_device_at(g._ctx, null, null, 0, 0, 0, 0, 0),
        "hulk_flush_batch": lambda: L_.hulk_flush_batch(g._ctx, 1),
        "hulk_flush_batch_after": lambda: L_.hulk_flush_batch_after(g._ctx, 1, null),
        "hulk_comm_init_loopback": lambda: L_.hulk_comm_init_loopback(g._ctx, 0, 2),
        "hulk_comm_init_host": lambda: L_.hulk_comm_init_host(g._ctx, 0, 2, _lib.EXCHANGE_FN(lambda *a: 0), None),
        "hulk_step_sharded": lambda: L_.hulk_step_sharded(g._ctx, null, null, 0, 0, 0, 1),
        "hulk_step_sharded_host": lambda: L_.hulk_step_sharded_host(g._ctx, null, null, 0, 1),
        "hulk_step_sliced": lambda: L_.hulk_step_sliced(g._ctx, null, null, 0, 0, 0, 0, 1),
    }
    for name, call in refused.items():
        assert call() == STATE, name
        assert b"snapshots" in L_.hulk_last_error(g._ctx), name
    g.add_reads(*stream(2 * I))                                      # the context is still good for what it is for
    g.finish()
    assert g.snapshot_count() == (2, 0)
    g.close()


# ---- 9. the CLI --------------------------------------------------------------------------------------------------------------
def run_cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "hulk_amd"] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("with_stream", [False, True])
def test_cli_stream_every(tmp_path, with_stream):
    from hulk_amd.sketchio import load_hulk_data
    lm, lw = library_trajectory("nodrift")
    S = CONFIGS["nodrift"]["S"]
    fq = str(tmp_path / "stream.fq")
    write_fastq(fq)
    base = ["sketch", "-f", fq, "-k", str(K), "-w", str(W), "-s", str(S), "-i", str(I)]
    r0 = run_cli(base + ["-o", "plain"], str(tmp_path))
    assert r0.returncode == 0, r0.stdout + r0.stderr
    r = run_cli(base + ["-o", "traj", "--streamEvery", "1"] + (["--stream"] if with_stream else []), str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "traj.json").read() == open(tmp_path / "plain.json").read()
    sdir = tmp_path / "traj.snapshots"
    names = sorted(os.listdir(sdir))
    assert names == ["%08d.json" % o for o in range(1, N_INT + 1)]
    final = json.load(open(tmp_path / "traj.json"))
    docs = []
    for t, nm in enumerate(names):
        d = load_hulk_data(str(sdir / nm))                          # (class, version, MD5 checks)
        (algo, hs), = d.signatures
        assert algo == "histosketch" and d.filename == final["filename"] and d.banner_label == final["banner_label"]
        assert np.array_equal(hs.mins, lm[t]) and np.array_equal(bits(hs.weights), bits(lw[t])), f"snapshot file {nm}"
        docs.append(json.load(open(sdir / nm)))
    if with_stream:
        lines = r.stdout.splitlines()
        assert len(lines) == N_INT
        assert [json.loads(x) for x in lines] == docs
        assert os.path.exists(tmp_path / "traj.log")
    else:
        assert not any(x.startswith("{") for x in r.stdout.splitlines())
    rs = run_cli(["smash", "-k", str(K), "-d", str(sdir), "-o", "m"], str(tmp_path))
    assert rs.returncode == 0, rs.stdout + rs.stderr
    from hulk_amd.smash import go_format_f2
    rows = open(tmp_path / "m.hulk-matrix.csv").read().splitlines()
    assert rows[0] == ",".join(str(sdir / nm) for nm in names), "the matrix is not in stream order"
    om, ow = oracle_trajectory("nodrift")
    want = pyorc.smash_matrix(om, ow, "jaccard")                    # (jaccard: only the mins enter)
    assert want.shape == (N_INT, N_INT) and len(rows) == N_INT + 1
    for t, line in enumerate(rows[1:]):
        assert line == ",".join(go_format_f2(100 - v * 100) for v in want[t]), f"row {t} of the trajectory's similarity matrix"


def test_cli_stream_every_needs_an_interval(tmp_path):
    fq = str(tmp_path / "stream.fq")
    write_fastq(fq)
    r = run_cli(["sketch", "-f", fq, "-k", str(K), "-o", "x", "--streamEvery", "2"], str(tmp_path))
    assert r.returncode == 1
    assert r.stdout.rstrip().endswith("ERROR---> --streamEvery needs an interval (-i)")
    assert not os.path.exists(tmp_path / "x.json") and not os.path.exists(tmp_path / "x.snapshots")


# ---- 10. the C++ host --------------------------------------------------------------------------------------------------------
def build_cpp_driver(tmp_path):
    libdir = os.path.join(ROOT, "hulk_amd", "csrc")
    exe = str(tmp_path / "snapshot_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "snapshot_driver.cpp"), "-o", exe,
           "-L", libdir, "-lhulkhip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name", ["nodrift", "decay"])
def test_cpp_host_matches_the_python_binding(name, tmp_path):
    """hulk::Boss::EnableSnapshots / CollectSnapshots / OnSnapshot (include/hulk.hpp) against GpuSketcher.snapshots()."""
    c = CONFIGS[name]
    exe = build_cpp_driver(tmp_path)
    bases, _ = stream()
    txt = tmp_path / "reads.txt"
    txt.write_bytes(b"\n".join(r.tobytes() for r in bases.reshape(-1, L)) + b"\n")
    g = sketcher(name)
    g.add_reads(*stream())
    g.finish()
    info, mins, weights = g.snapshots()
    fm, fw = g.sketch()
    g.close()
    args = [str(txt), str(K), str(W), str(c["S"]), str(I), repr(c["decay"]), "1"]
    for mode, cap in (("collect", "64"), ("callback", "4")):
        p = subprocess.run([exe, mode] + args + [cap], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        docs = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
        final, docs = docs[-1], docs[:-1]
        assert [{"ordinal": d["ordinal"], "n_reads": d["n_reads"]} for d in docs] == info, mode
        assert all(d["ksize"] == K and d["bins"] == K ** 4 and d["drift"] == (c["decay"] != 1.0) for d in docs)
        assert_bitwise(np.array([d["mins"] for d in docs], dtype=np.uint64), np.array([d["weights"] for d in docs]), mins, weights,
                       f"{name} {mode}")                              # (%.17g round-trips)
        assert final["delivered"] == (N_INT if mode == "callback" else 0)
        assert np.array_equal(np.array(final["mins"], dtype=np.uint64), fm) and np.array_equal(bits(np.array(final["weights"])), bits(fw))
    p = subprocess.run([exe, "throw"] + args + ["64"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 3 and p.stdout.strip().splitlines()[-1] == "runtime_error|third snapshot|seen", p.stdout[-500:] + p.stderr[-500:]
