"""The steady flush: once k_flush_decide has passed over a whole batch, the host (which learns the verdict from the word the
kernel stores to its memory) queues k_count_used, k_flush_decide, k_cms_steady_sums, k_cms_steady_add instead of the full
chain.  Comparator: a HULK_FLAG_NO_SKIP context, which never goes steady, fed the same calls; yardstick: oracle/pyorc.
Shapes: k = 15, w = 9, interval 2000, batch 4 — a batch of uniform reads fills every count-min counter, so from the second
batch on k_flush_decide passes over (tests/test_gpu_snapshots.py, test_batches_the_flush_skips_still_record)."""
import functools

import numpy as np
import pytest

from oracle import pyorc

pytestmark = pytest.mark.gpu

K, W, I, T, L = 15, 9, 2000, 4, 150
BATCH = T * I
WEIGHT_RTOL = 1e-9
STEADY = ("k_cms_steady_sums", "k_cms_steady_add")
FULL_ONLY = ("k_cms_segsum", "k_cms_base", "k_cms_freq")
TAIL = 2 * I + 700                      # a last batch of two intervals, and a partial interval closed by finish()


def lib():
    from hulk_amd import _lib
    return _lib


def sketcher(S, flags=0, **kw):
    import hulk_amd
    return hulk_amd.GpuSketcher(K, W, S, kw.pop("interval", I), kw.pop("decay", 1.0), batch=T, flags=flags, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def reads(first, n):
    from hulk_amd import synth
    bases, offsets = synth.reads_numpy(first, n, L)
    bases.setflags(write=False); offsets.setflags(write=False)
    return bases, offsets


def results(g):
    m, w = g.sketch()
    return dict(mins=m, weights=w, cms=g.cms(), counters=g.counters(), hist=g.histogram())


def assert_same_bits(a, b, what):
    assert np.array_equal(a["mins"], b["mins"]), f"{what}: mins"
    assert np.array_equal(bits(a["weights"]), bits(b["weights"])), f"{what}: weights"
    assert np.array_equal(a["cms"], b["cms"]), f"{what}: count-min counters"
    assert a["counters"] == b["counters"], f"{what}: counters"
    assert np.array_equal(a["hist"], b["hist"]), f"{what}: spectrum"


def ragged_stream(g):
    """two batches, a synchronisation, two more batches and the ragged tail; finish().  Flushes: 2 before the synchronisation,
    4 after it (two whole batches, one of two intervals, the partial interval of finish())."""
    g.add_reads(*reads(0, 2 * BATCH))
    g.synchronize()
    g.add_reads(*reads(2 * BATCH, 2 * BATCH + TAIL))
    g.finish()


@functools.lru_cache(maxsize=None)
def ragged_oracle(S):
    o = pyorc.Sketcher(K, W, S, 0, 1.0, I)
    o.add_reads(*reads(0, 2 * BATCH))
    o.add_reads(*reads(2 * BATCH, 2 * BATCH + TAIL))
    o.finish()
    m, w = o.sketch()
    out = dict(mins=m, weights=w, cms=o.cms(), counters=o.counters())
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def ragged_one_stream(S):
    """case 1's two contexts: (steady: results, profile table), (HULK_FLAG_NO_SKIP: results, profile table)"""
    out = []
    for extra in (0, lib().HULK_FLAG_NO_SKIP):
        g = sketcher(S, lib().HULK_FLAG_NO_OVERLAP | extra)
        g.set_profiling(32)
        ragged_stream(g)
        tbl = g.profile_table()
        out.append((results(g), tbl))
        g.close()
    return out


@pytest.mark.parametrize("S", [16, 64])
def test_adoption_and_equality(S):
    (got, tbl), (ref, ref_tbl) = ragged_one_stream(S)
    print({k: v[0] for k, v in tbl.items()})
    assert_same_bits(got, ref, "steady against HULK_FLAG_NO_SKIP")
    assert not got["hist"].any(), "the ring is not wiped"
    want = ragged_oracle(S)
    assert np.array_equal(got["mins"], want["mins"]) and np.array_equal(got["cms"], want["cms"])
    assert got["counters"] == {key: want["counters"][key] for key in got["counters"]}
    assert np.allclose(got["weights"], want["weights"], rtol=WEIGHT_RTOL, atol=0)
    # the full chain for the two flushes in front of the synchronisation, the steady chain for the four behind it
    assert tbl["k_count_used"][0] == tbl["k_flush_decide"][0] == 6
    for kname in FULL_ONLY + ("k_scan_test", "k_cws_apply"):
        assert tbl[kname][0] == 2, (kname, tbl[kname])
    for kname in STEADY:
        assert tbl[kname][0] == 4 and tbl[kname][1] > 0, (kname, tbl.get(kname))
    assert not any(kname in ref_tbl for kname in STEADY) and ref_tbl["k_cms_freq"][0] == 6


@pytest.mark.parametrize("S", [16, 64])
def test_overlapped_equality(S):
    g = sketcher(S)                      # two work lanes, flushes on their own stream
    ragged_stream(g)
    got = results(g)
    g.close()
    assert_same_bits(got, ragged_one_stream(S)[0][0], "overlapped against one stream")


def steady_launches(g, more):
    """two batches, a synchronisation, `more` (a callable) — the steady kernels the profile table then holds"""
    g.set_profiling(32)
    g.add_reads(*reads(0, 2 * BATCH))
    g.synchronize()
    more(g)
    tbl = g.profile_table()
    assert tbl["k_flush_decide"][0] >= 3
    return {k: tbl[k][0] for k in STEADY if k in tbl}


@pytest.mark.parametrize("name", ["no_skip", "no_prune", "decay", "snapshots"])
def test_nothing_to_adopt(name):
    f = lib()
    kw = {"no_skip": dict(flags=f.HULK_FLAG_NO_SKIP), "no_prune": dict(flags=f.HULK_FLAG_NO_PRUNE), "decay": dict(decay=0.02),
          "snapshots": dict(snapshots=1, snapshot_capacity=64)}[name]
    g = sketcher(16, kw.pop("flags", 0) | f.HULK_FLAG_NO_OVERLAP, **kw)
    got = steady_launches(g, lambda g: g.add_reads(*reads(2 * BATCH, 2 * BATCH)))
    g.close()
    assert got == {}


def test_a_stream_that_still_passes_is_not_adopted():
    """Every interval is the same 40 reads 50 times over: about 1100 of the 50625 bins, above the 1 % rule, but a count-min
    row has 2000 counters — some stay at zero, k_flush_decide's m is 0 and every verdict is "pass"."""
    few = reads(0, 40)[0]
    bases = np.tile(few, 2 * BATCH // 40)
    offsets = np.arange(2 * BATCH + 1, dtype=np.uint64) * np.uint64(L)
    o = pyorc.Sketcher(K, W, 16, 0, 1.0, I)
    o.add_reads(bases, offsets)
    used, ctr_min = int((o.cms() != 0).sum()), o.cms().min()
    o.close()
    assert ctr_min == 0 and used > 0, "the stream does not do what the test needs: the oracle's counters have no zero left"
    g = sketcher(16, lib().HULK_FLAG_NO_OVERLAP)
    g.set_profiling(32)
    g.add_reads(bases, offsets)
    g.synchronize()
    g.add_reads(bases, offsets)
    g.finish()                            # (raises if an interval fell under the 1 % rule)
    tbl = g.profile_table()
    g.close()
    assert tbl["k_cms_freq"][0] == tbl["k_flush_decide"][0] == 5 and not any(k in tbl for k in STEADY)


def test_the_one_percent_rule_in_steady_state():
    import hulk_amd
    one = reads(7, 1)[0]
    sparse = (np.tile(one, I), np.arange(I + 1, dtype=np.uint64) * np.uint64(L))     # an interval of one read: ~27 bins
    out = []
    for extra in (0, lib().HULK_FLAG_NO_SKIP):
        g = sketcher(16, lib().HULK_FLAG_NO_OVERLAP | extra)
        g.set_profiling(32)
        g.add_reads(*reads(0, 2 * BATCH))
        g.synchronize()
        g.flush()                         # a spectrum without a used bin: skipped silently (boss.go:118)
        g.synchronize()
        silent = results(g)
        g.add_reads(*sparse)
        with pytest.raises(hulk_amd.HulkError, match="not used yet"):
            g.finish()
        tbl = g.profile_table()
        out.append((silent, g.cms(), g.counters(), tbl))
        g.close()
    (silent, cms, counters, tbl), (ref_silent, ref_cms, ref_counters, ref_tbl) = out
    assert_same_bits(silent, ref_silent, "after the empty flush")
    assert np.array_equal(cms, ref_cms) and counters == ref_counters
    assert np.array_equal(cms, silent["cms"]), "the interval under the 1 % rule reached the counters"
    assert all(tbl[k][0] >= 2 for k in STEADY) and not any(k in ref_tbl for k in STEADY)


def test_add_histogram_and_flush_after_adoption():
    rng = np.random.default_rng(5)
    hist = np.where(rng.random(K ** 4) < 0.3, rng.integers(1, 50, K ** 4), 0).astype(np.uint32)
    out = []
    for extra in (0, lib().HULK_FLAG_NO_SKIP):
        g = sketcher(16, lib().HULK_FLAG_NO_OVERLAP | extra)
        g.set_profiling(32)
        g.add_reads(*reads(0, 2 * BATCH))
        g.synchronize()
        g.add_histogram(hist)
        g.flush()
        g.finish()
        tbl = g.profile_table()
        out.append((results(g), tbl))
        g.close()
    (got, tbl), (ref, ref_tbl) = out
    assert_same_bits(got, ref, "hulk_add_histogram + hulk_flush")
    assert not got["hist"].any()
    assert all(tbl[k][0] >= 1 for k in STEADY) and not any(k in ref_tbl for k in STEADY)
