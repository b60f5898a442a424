"""The steady flush adds the batch's spectra per bin first and runs the count-min once over the sum (k_cms_steady_sums,
k_cms_steady_add: "The steady flush", hulk_countmin.hip).  What that must not change, at the places where it can go wrong: a
ring base that moves and wraps, a spectrum of the batch that does not go, sums wider than 32 bits, bins next to the borders
of the kernels' bin segments.  Comparator: a HULK_FLAG_NO_SKIP context, which never goes steady, fed the same calls, bit for
bit; yardstick: oracle/pyorc.  Shapes as tests/test_gpu_flush_steady.py: k = 15 (50,625 bins, odd: ring slots 1 to 4 do not
start on a 16-byte boundary), w = 9, interval 2000, batch 4 (a ring of 5), S = 16.  Every case goes steady first: two batches,
then a synchronisation."""
import functools

import numpy as np
import pytest

from oracle import pyorc

pytestmark = pytest.mark.gpu

K, W, I, T, L, S = 15, 9, 2000, 4, 150, 16
B = K ** 4
BATCH = T * I
ADOPT = 2 * BATCH
WEIGHT_RTOL = 1e-9
STEADY = ("k_cms_steady_sums", "k_cms_steady_add")


def lib():
    from hulk_amd import _lib
    return _lib


def sketcher(flags=0):
    import hulk_amd
    return hulk_amd.GpuSketcher(K, W, S, I, 1.0, batch=T, flags=flags)


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


def assert_oracle(got, want, what):
    assert np.array_equal(got["mins"], want["mins"]), f"{what}: mins against the oracle"
    assert np.array_equal(got["cms"], want["cms"]), f"{what}: count-min against the oracle"
    assert got["counters"] == {key: want["counters"][key] for key in got["counters"]}, f"{what}: counters against the oracle"
    assert np.allclose(got["weights"], want["weights"], rtol=WEIGHT_RTOL, atol=0), f"{what}: weights against the oracle"


def run_pair(more, overlapped=False):
    """[(results, profile table)] of the steady context and of the HULK_FLAG_NO_SKIP comparator: adoption, then `more(g)`"""
    out = []
    for extra in (0, lib().HULK_FLAG_NO_SKIP):
        g = sketcher((0 if overlapped else lib().HULK_FLAG_NO_OVERLAP) | extra)
        g.set_profiling(32)
        g.add_reads(*reads(0, ADOPT))
        g.synchronize()
        try:
            more(g)
            tbl = g.profile_table()
            out.append((results(g), tbl))
        finally:
            g.close()
    (got, tbl), (ref, ref_tbl) = out
    if not overlapped:
        assert all(tbl.get(k, (0,))[0] >= 1 for k in STEADY), "the context did not go steady"
    assert not any(k in ref_tbl for k in STEADY)
    return got, ref


def run_oracle(more):
    o = pyorc.Sketcher(K, W, S, 0, 1.0, I)
    try:
        o.add_reads(*reads(0, ADOPT))
        more(o)
        m, w = o.sketch()
        return dict(mins=m, weights=w, cms=o.cms(), counters=o.counters())
    finally:
        o.close()


# ---- case 1: a ring base that moves.  Six calls of 5,000 reads (2.5 intervals): flushes of 2 and 3 spectra from ring bases 0
# and 2, a pending half interval across every other call.  In a ring of 5 those never pass its end (2 + 3 = 5 and a call that
# ends on an interval border starts the next ring at 0), so the same with calls of 4,500 reads: the flushes are slots 0 1,
# 2 3, 4 0 — wrapped —, 1 2 3, 0 1, 2 3, and finish() closes slot 4.
CALLS = 6


def moving_base(call_reads, g):
    for i in range(CALLS):
        g.add_reads(*reads(ADOPT + i * call_reads, call_reads))
    g.finish()


@functools.lru_cache(maxsize=None)
def moving_base_one_stream(call_reads):
    return run_pair(functools.partial(moving_base, call_reads))


@pytest.mark.parametrize("call_reads", [5000, 4500])
def test_moving_ring_base_one_stream(call_reads):
    got, ref = moving_base_one_stream(call_reads)
    assert_same_bits(got, ref, "steady against HULK_FLAG_NO_SKIP")
    assert not got["hist"].any(), "the ring is not wiped"
    assert_oracle(got, run_oracle(functools.partial(moving_base, call_reads)), "moving ring base")


@pytest.mark.parametrize("call_reads", [5000, 4500])
def test_moving_ring_base_overlapped(call_reads):
    got, ref = run_pair(functools.partial(moving_base, call_reads), overlapped=True)
    assert_same_bits(got, ref, "overlapped: steady against HULK_FLAG_NO_SKIP")
    assert_same_bits(got, moving_base_one_stream(call_reads)[0], "overlapped against one stream")
    assert not got["hist"].any(), "the ring is not wiped"


# ---- case 2: one call of four intervals, the third one read 2000 times over (about 27 bins: under 1 % of 50,625)
def test_one_sparse_interval_inside_a_batch():
    import hulk_amd
    one = reads(7, 1)[0]
    parts = [reads(ADOPT, I)[0], reads(ADOPT + I, I)[0], np.tile(one, I), reads(ADOPT + 2 * I, I)[0]]
    bases = np.concatenate(parts)
    offsets = np.arange(4 * I + 1, dtype=np.uint64) * np.uint64(L)

    def more(g):
        g.add_reads(bases, offsets)
        with pytest.raises(hulk_amd.HulkError, match="not used yet"):
            g.finish()

    got, ref = run_pair(more)
    assert np.array_equal(got["cms"], ref["cms"]) and got["counters"] == ref["counters"]
    # the three intervals that go, and only they: the oracle fed the stream without the sparse interval
    want = run_oracle(lambda o: (o.add_reads(*reads(ADOPT, 3 * I)), o.finish()))
    assert np.array_equal(got["cms"], want["cms"]), "count-min: not exactly the three intervals above the 1 % rule"
    assert np.array_equal(ref["cms"], want["cms"])


# ---- case 3: sums wider than 32 bits.  Every bin 2^27: a row gains 50,625 * 2^27 and the counters that 32 or more bins map
# to gain 2^32 or more (the largest 47 bins: 6,308,233,216); the oracle's counters are float64 and exact far beyond that.
def test_wide_sums():
    hist = np.full(B, 1 << 27, dtype=np.uint32)

    def more(g):
        g.add_histogram(hist)
        g.flush()
        g.finish()

    before = run_oracle(lambda o: None)["cms"]
    want = run_oracle(more)
    gain = want["cms"] - before
    print("counters gaining >= 2^32:", int((gain >= 2.0 ** 32).sum()), "largest gain:", int(gain.max()))
    assert (gain.sum(axis=1) == float(B) * 2.0 ** 27).all() and gain.max() >= 2.0 ** 32, "the oracle does not take the case"
    got, ref = run_pair(more)
    assert np.array_equal(ref["cms"], want["cms"]), "precondition: the comparator does not equal the oracle"
    assert_same_bits(got, ref, "wide sums")
    assert_oracle(got, want, "wide sums")
    assert not got["hist"].any()


# ---- case 4: bins at the edges.  600 used bins (1.2 %: the spectrum goes): bin 0, bin B - 1, the two bins on either side of
# every border between the bin segments of k_cms_steady_add — cms_fold_seg_bins (hulk_countmin.hip) for the 16 segments it ships
# with and the 4 and 8 of its sweep — and of the 16 segments of cms_seg_chunks (the HULK_STEADY_SEGSUM form and the full chain).
def segment_borders():
    borders = set()
    for segs in (4, 8, 16):
        seg_bins = (((B + segs - 1) // segs) + 255) & ~255
        borders.update(range(seg_bins, B, seg_bins))
    seg_chunks = ((B + 63) // 64 + 15) // 16
    borders.update(range(seg_chunks * 64, B, seg_chunks * 64))
    return sorted(borders)


def test_bins_at_the_edges():
    rng = np.random.default_rng(11)
    edge = {0, B - 1}
    for b in segment_borders():
        edge.update((b - 1, b))
    assert len(edge) < 600
    rest = rng.choice(np.setdiff1d(np.arange(B), sorted(edge)), 600 - len(edge), replace=False)
    used = np.concatenate([np.fromiter(edge, dtype=np.int64), rest])
    hist = np.zeros(B, dtype=np.uint32)
    hist[used] = rng.integers(1, 1000, len(used))
    assert (hist != 0).sum() == 600

    def more(g):
        g.add_histogram(hist)
        g.flush()
        g.finish()

    got, ref = run_pair(more)
    assert_same_bits(got, ref, "bins at the edges")
    assert_oracle(got, run_oracle(more), "bins at the edges")
    assert not got["hist"].any()
