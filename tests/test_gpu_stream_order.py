"""The stream-order contract of the device entry points (include/hulk_hip.h): a context on the caller's stream
(hulk_set_stream, GpuSketcher(stream=...)), hulk_add_reads_device with buffers produced on that stream, hulk_bin_reads_device
with the spectra read on it through hulk_histogram_device, and hulk_flush_batch_after behind a collective on a second stream.
The code under test is event plumbing (hulk_flush.hip: ev_fork, lanes_join, ev_binned), so every flow is built to make a missing
wait change the result:

  * the bases arrive LATE: on the caller's stream each batch queues torch.cuda._sleep (~30 ms, calibrated here and asserted
    to be >= 10 x one batch's whole call chain), then the copy of the batch from pinned memory, then the library call — and
    no host synchronisation anywhere in the loop;
  * until that copy lands the buffer holds DECOYS: valid ACGT reads of the same lengths from another seed, so a kernel that
    runs too early reads initialised, in-bounds, wrong data.  The offsets are uploaded and synchronised once, up front:
    only bases are ever late (a safety rule: lengths never come from a buffer in flight);
  * before the GPU is touched the oracle alone shows that the decoy stream gives another count-min and another sketch, and,
    for the collective, that the stream without the other rank's intervals gives another count-min (its sketch cannot
    differ at these shapes: inputs_are_a_test): "the inputs are no test" otherwise.

Yardsticks of every flow: oracle/pyorc over the same global stream (mins, count-min counters equal; weights rtol 1e-9);
a context on its private stream fed the same calls with torch.cuda.synchronize() in front of each (bit-identical mins,
weight bits, cms, counters, spectrum); the same with HULK_FLAG_NO_SKIP (which flush chain ran does not matter).
Shapes: those of tests/test_gpu_flush_steady.py — k = 15, w = 9, S = 16, interval 2000, batch 4, uniform 150-base reads of
hulk_amd.synth; six batches per flow (each ring and work lane three times; the steady flush is open from batch 2 on)."""
import functools

import numpy as np
import pytest

from oracle import pyorc

pytestmark = pytest.mark.gpu

K, W, S, I, T, L = 15, 9, 16, 2000, 4, 150
B = K ** 4
BATCH = T * I
NB = 6                                  # batches per flow
TAIL = 2 * I + 700                      # a last call of two intervals and a partial one that finish() closes
N = NB * BATCH + TAIL
EVEN = (BATCH,) * NB + (TAIL,)
UNEVEN = (1400, 5200, 10200, 2600, 8000, 12800, 7300, 5200)     # 0.7 I, 2.6 I, 5.1 I, ...: flushes start at ring_base != 0
assert sum(UNEVEN) == sum(EVEN) == N
MAXCALL = max(UNEVEN)
WEIGHT_RTOL = 1e-9
DECOY_SEED = 0x4445434F
DELAY_MS = 30.0
DOMINATES = 10.0                        # the delay against one batch's call chain
OFFS = np.arange(MAXCALL + 1, dtype=np.uint64) * np.uint64(L)


def lib():
    from hulk_amd import _lib
    return _lib


def sketcher(flags=0, **kw):
    import hulk_amd
    return hulk_amd.GpuSketcher(K, W, S, I, 1.0, batch=T, flags=flags, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# the streams on the host, the oracle, and what the inputs have to be for the tests to mean anything

@functools.lru_cache(maxsize=None)
def real():
    from hulk_amd import synth
    bases = synth.reads_numpy(0, N, L)[0]
    bases.setflags(write=False)
    return bases


@functools.lru_cache(maxsize=None)
def decoy():
    from hulk_amd import synth
    bases = synth.reads_numpy(0, MAXCALL, L, seed=DECOY_SEED)[0]
    bases.setflags(write=False)
    return bases


def pieces(calls):
    """the global stream cut into calls: [(first read, reads)]"""
    at, out = 0, []
    for n in calls:
        out.append((at, n)); at += n
    return out


def own_half(b):
    """first read of the two intervals of batch b this "rank" bins; the other rank's are the two behind them"""
    return b * BATCH


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the interval rule over: "whole" — the N reads; "six" — the NB whole batches; "decoy_even" / "decoy_uneven" / "decoy_six" —
    what the buffer holds before each late copy, call by call; "own_half" — the six batches without the other rank's intervals"""
    if name == "whole": parts = [real()]
    elif name == "six": parts = [real()[:NB * BATCH * L]]
    elif name == "decoy_even": parts = [decoy()[:n * L] for n in EVEN]
    elif name == "decoy_uneven": parts = [decoy()[:n * L] for n in UNEVEN]
    elif name == "decoy_six": parts = [decoy()[:BATCH * L]] * NB
    elif name == "own_half": parts = [real()[own_half(b) * L:(own_half(b) + 2 * I) * L] for b in range(NB)]
    else: raise KeyError(name)
    o = pyorc.Sketcher(K, W, S, 0, 1.0, I)
    for p in parts:
        for at in range(0, len(p) // L, MAXCALL):
            n = min(MAXCALL, len(p) // L - at)
            o.add_reads(p[at * L:(at + n) * L], OFFS[:n + 1])
    o.finish()
    m, w = o.sketch()
    out = dict(mins=m, weights=w, cms=o.cms(), counters=o.counters())
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def interval_spectra():
    """uint32[NB * T][B]: the k-mer spectrum of every interval of the six batches (the oracle's binning, no flush)"""
    o = pyorc.Sketcher(K, W, 1, 0, 1.0, 0)
    out = np.zeros((NB * T, B), dtype=np.uint32)
    for i in range(NB * T):
        o.add_reads(real()[i * I * L:(i + 1) * I * L], OFFS[:I + 1])
        out[i] = o.histogram().astype(np.uint32)
        o.wipe()
    o.close()
    return out


def inputs_are_a_test(right, *wrong, sketch=True):
    """CPU only: every stream a mis-ordered run would sketch gives another count-min and another sketch than the right one.
    sketch=False — the stream without the other rank's intervals: another count-min only.  At these shapes the sketch cannot
    tell: the CWS weights are negative (about -3) and A = K / f only falls for a SMALLER estimate f, the counters only grow,
    so the 16 slots are settled by the first interval of the stream (the oracle: not one min or weight changes in intervals
    1..9) — and that interval is this rank's.  The count-min counters, which every flow compares with the oracle's for
    equality, are what shows a flush that did not wait (12 of 24 intervals missing: every counter lower)."""
    a = oracle(right)
    for name in wrong:
        b = oracle(name)
        assert not np.array_equal(a["cms"], b["cms"]), f"the inputs are no test: {name} counts like {right}"
        if sketch:
            assert not np.array_equal(a["mins"], b["mins"]) or not np.array_equal(bits(a["weights"]), bits(b["weights"])), \
                f"the inputs are no test: {name} sketches like {right}"


# ---------------------------------------------------------------------------------------------------------------------------
# comparisons

def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def results(g):
    m, w = g.sketch()
    return dict(mins=m, weights=w, cms=g.cms(), counters=g.counters(), hist=g.histogram())


def assert_same_bits(a, b, what):
    assert np.array_equal(a["mins"], b["mins"]), f"{what}: mins"
    assert np.array_equal(bits(a["weights"]), bits(b["weights"])), f"{what}: weights"
    assert np.array_equal(a["cms"], b["cms"]), f"{what}: count-min counters"
    assert a["counters"] == b["counters"], f"{what}: counters"
    assert np.array_equal(a["hist"], b["hist"]), f"{what}: spectrum"


def assert_oracle(got, want, counters=True):
    assert np.array_equal(got["cms"], want["cms"]), "count-min counters against the oracle"
    assert np.array_equal(got["mins"], want["mins"]), "mins against the oracle"
    assert np.allclose(got["weights"], want["weights"], rtol=WEIGHT_RTOL, atol=0), "weights against the oracle"
    if counters:
        assert got["counters"] == {key: want["counters"][key] for key in got["counters"]}
    assert not got["hist"].any(), "the ring is not wiped"


def assert_three_yardsticks(got, oracle_name, ref_name, counters=True):
    assert_oracle(got, oracle(oracle_name), counters)
    assert_same_bits(got, reference(ref_name, 0), "against the synchronised private-stream context")
    assert_same_bits(got, reference(ref_name, lib().HULK_FLAG_NO_SKIP), "against the synchronised HULK_FLAG_NO_SKIP context")


# ---------------------------------------------------------------------------------------------------------------------------
# device side

@functools.lru_cache(maxsize=None)
def constants():
    """(decoys, offsets) in device memory — uploaded and synchronised once; nothing ever writes them again"""
    import torch
    d = torch.from_numpy(decoy().copy()).cuda()
    off = torch.from_numpy(OFFS.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    return d, off


@functools.lru_cache(maxsize=None)
def pinned(first, n):
    import torch
    return torch.from_numpy(real()[first * L:(first + n) * L].copy()).pin_memory()


class Buffers:
    """The one bases buffer of a flow (the decoys in it, the tail zeroed) and the constants."""
    def __init__(self):
        import torch
        self.decoy, self.offs = constants()
        self.bases = torch.zeros(((MAXCALL * L + 15) // 8) * 8, dtype=torch.uint8, device="cuda")
        self.bases[:MAXCALL * L].copy_(self.decoy)
        torch.cuda.synchronize()

    def args(self, n):
        return self.bases.data_ptr(), self.offs.data_ptr(), n, L, self.bases.numel()


def caller_stream(kind):
    """(torch stream, the handle hulk_set_stream takes)"""
    import torch
    if kind == "null":
        s = torch.cuda.default_stream()
        assert s.cuda_stream == 0, "torch's default stream is not the HIP null stream here"
        return s, 0
    s = torch.cuda.Stream()
    return s, s.cuda_stream


def late(buf, xs, first, n, call, decoys_after=True):
    """On the caller's stream: the delay, the batch's bases from pinned memory, the library call and — the header allows it
    once the stream has passed the call — the decoys again.  The host waits for nothing."""
    import torch
    cycles = delay()[0]
    with torch.cuda.stream(xs):
        torch.cuda._sleep(cycles)
        buf.bases[:n * L].copy_(pinned(first, n), non_blocking=True)
    call(*buf.args(n))
    if decoys_after:
        with torch.cuda.stream(xs):
            buf.bases[:n * L].copy_(buf.decoy[:n * L], non_blocking=True)


def synced(buf, first, n, call):
    """The same call for a context on its private stream: the device idle in front of the copy and in front of the call."""
    import torch
    torch.cuda.synchronize()
    buf.bases[:n * L].copy_(pinned(first, n), non_blocking=True)
    torch.cuda.synchronize()
    call(*buf.args(n))


class Spectra:
    """hulk_histogram_device() as a zero-copy [rows][B] view for torch.as_tensor (declared int32: the same 32 bits)."""
    def __init__(self, ptr, rows):
        self.__cuda_array_interface__ = {"shape": (rows, B), "typestr": "<i4", "data": (int(ptr), False), "version": 2}


def spectra_view(g, rows=T):
    import torch
    v = torch.as_tensor(Spectra(g.histogram_device_ptr(), rows), device="cuda")
    assert v.data_ptr() == g.histogram_device_ptr(), "torch copied the spectra instead of viewing them"
    return v


@functools.lru_cache(maxsize=None)
def delay():
    """(cycles of torch.cuda._sleep for ~DELAY_MS, that delay as measured, one batch's whole call chain as measured) — ms between
    events on one stream.  The chain is a HULK_FLAG_NO_OVERLAP context's: binning AND flush on the caller's stream, the full
    flush chain every time (such a context adopts the steady one only when synchronised)."""
    import torch
    xs = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(10)]
    probe = 4_000_000
    with torch.cuda.stream(xs):
        torch.cuda._sleep(1000)
        ev[0].record(); torch.cuda._sleep(probe); ev[1].record()
    xs.synchronize()
    cycles = max(int(probe * DELAY_MS / ev[0].elapsed_time(ev[1])), 1)
    with torch.cuda.stream(xs):
        ev[2].record(); torch.cuda._sleep(cycles); ev[3].record()
    xs.synchronize()
    delay_ms = ev[2].elapsed_time(ev[3])
    buf = Buffers()
    buf.bases[:BATCH * L].copy_(pinned(0, BATCH))
    torch.cuda.synchronize()
    g = sketcher(lib().HULK_FLAG_NO_OVERLAP, stream=xs.cuda_stream)
    chain = []
    for i in range(3):                  # (the first call builds what every later one finds in place: printed, not used)
        with torch.cuda.stream(xs):
            ev[4 + 2 * i].record()
        g.add_reads_device(*buf.args(BATCH))
        with torch.cuda.stream(xs):
            ev[5 + 2 * i].record()
    xs.synchronize()
    chain = [ev[4 + 2 * i].elapsed_time(ev[5 + 2 * i]) for i in range(3)]
    g.close()
    chain_ms = max(chain[1:])
    print(f"stream order: delay {delay_ms:.3f} ms ({cycles} cycles), batch call chain {chain_ms:.3f} ms "
          f"(first call {chain[0]:.3f} ms), ratio {delay_ms / chain_ms:.1f}")
    assert delay_ms >= DOMINATES * chain_ms, f"the delay ({delay_ms:.3f} ms) does not dominate a batch ({chain_ms:.3f} ms): the tests prove nothing"
    return cycles, delay_ms, chain_ms


# ---------------------------------------------------------------------------------------------------------------------------
# the synchronised comparators (yardsticks 2 and 3), one per flow and flag set

def add_calls(g, buf, calls, feed):
    for first, n in pieces(calls):
        feed(buf, first, n, g.add_reads_device)


@functools.lru_cache(maxsize=None)
def other_rank_spectra():
    """int32 [NB][2][B] in device memory: the spectra of intervals 2 and 3 of every batch, binned beforehand by a synchronised
    helper context — what the collective delivers."""
    import torch
    out = torch.zeros((NB, 2, B), dtype=torch.int32, device="cuda")
    buf = Buffers()
    g = sketcher()
    for b in range(NB):
        synced(buf, own_half(b) + 2 * I, 2 * I, lambda *a: g.bin_reads_device(*a, reads_per_spectrum=I))
        g.synchronize()
        out[b].copy_(spectra_view(g, 2))
        torch.cuda.synchronize()
        g.flush_batch(2)                # (wipes the ring; the helper's sketch is of no interest)
    g.finish()
    g.close()
    want = interval_spectra().reshape(NB, T, B)[:, 2:4]
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want), "the helper's spectra are not the oracle's"
    return out


@functools.lru_cache(maxsize=None)
def reference(flow, flags):
    import torch
    buf = Buffers()
    g = sketcher(flags)
    if flow in ("even", "uneven"):
        add_calls(g, buf, EVEN if flow == "even" else UNEVEN, synced)
    elif flow == "bin":
        for b in range(NB):
            synced(buf, b * BATCH, BATCH, lambda *a: g.bin_reads_device(*a, reads_per_spectrum=I))
            g.flush_batch(T)
    elif flow == "after":
        side = torch.cuda.Stream()
        for b in range(NB):
            synced(buf, own_half(b), 2 * I, lambda *a: g.bin_reads_device(*a, reads_per_spectrum=I))
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                spectra_view(g)[2:4].copy_(other_rank_spectra()[b])
            torch.cuda.synchronize()
            g.flush_batch(T, after_stream=side.cuda_stream)
    else:
        raise KeyError(flow)
    g.finish()
    out = results(g)
    g.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the cases

def test_the_delay_dominates_a_batch():
    cycles, delay_ms, chain_ms = delay()
    assert delay_ms >= DOMINATES * chain_ms


@pytest.mark.parametrize("config", ["two_lanes", "one_lane", "no_overlap"])
@pytest.mark.parametrize("kind", ["stream", "null"])
def test_add_reads_device_on_the_callers_stream(kind, config):
    """Case 1.  One buffer for all batches; right behind each call, on the same stream, the decoys go back into it (lanes_join
    is what makes that safe for lane 1), then the delay and the next batch's late copy."""
    inputs_are_a_test("whole", "decoy_even")
    xs, handle = caller_stream(kind)
    kw = {"two_lanes": dict(work_lanes=2), "one_lane": dict(work_lanes=1), "no_overlap": dict(flags=lib().HULK_FLAG_NO_OVERLAP)}[config]
    buf = Buffers()
    g = sketcher(stream=handle, **kw)
    add_calls(g, buf, EVEN, lambda buf, first, n, call: late(buf, xs, first, n, call))
    g.finish()
    got = results(g)
    g.close()
    assert_three_yardsticks(got, "whole", "even")


def test_uneven_call_boundaries_on_the_callers_stream():
    """Case 2.  Calls of 0.7, 2.6, 5.1, ... intervals: several launches per call, on either lane, flushes from ring_base != 0."""
    inputs_are_a_test("whole", "decoy_uneven")
    xs, handle = caller_stream("stream")
    buf = Buffers()
    g = sketcher(stream=handle)
    add_calls(g, buf, UNEVEN, lambda buf, first, n, call: late(buf, xs, first, n, call))
    g.finish()
    got = results(g)
    g.close()
    assert_three_yardsticks(got, "whole", "uneven")


def test_bin_reads_device_spectra_read_on_the_callers_stream():
    """Case 3.  Late bases, hulk_bin_reads_device, and — the stream busy for another delay first — a copy of the batch's spectra
    taken on the caller's stream through hulk_histogram_device(), then hulk_flush_batch: the copy has to see the whole binning
    (lane 1 joined) and has to be passed before the flush wipes what it reads.  The pointer: two values, alternating."""
    import torch
    inputs_are_a_test("six", "decoy_six")
    xs, handle = caller_stream("stream")
    buf = Buffers()
    g = sketcher(stream=handle)
    cycles = delay()[0]
    clones, ptrs = [], []
    for b in range(NB):
        late(buf, xs, b * BATCH, BATCH, lambda *a: g.bin_reads_device(*a, reads_per_spectrum=I))
        ptrs.append(g.histogram_device_ptr())
        with torch.cuda.stream(xs):
            torch.cuda._sleep(cycles)
            clones.append(spectra_view(g).clone())
        g.flush_batch(T)
    g.finish()
    got = results(g)
    g.close()
    print("hulk_histogram_device per batch:", [hex(p) for p in ptrs])
    assert ptrs[0] != ptrs[1] and all(ptrs[b] == ptrs[b % 2] for b in range(NB)), "the pointer does not alternate between two values"
    want = interval_spectra().reshape(NB, T, B)
    for b in range(NB):
        assert np.array_equal(clones[b].cpu().numpy().view(np.uint32), want[b]), f"the spectra of batch {b} as read on the caller's stream"
    assert_three_yardsticks(got, "six", "bin")


@pytest.mark.parametrize("mode", ["second_stream", "own_stream", "private_synchronised"])
def test_flush_batch_behind_a_collective(mode):
    """Case 4.  This context bins intervals 0 and 1 of every batch; the "collective" — the delay, then a copy of the other rank's
    spectra into rows 2 and 3 of hulk_histogram_device() — runs
      second_stream: on a stream D that waited for the context's stream A; hulk_flush_batch_after(D);
      own_stream: on A itself, hulk_flush_batch (steps (2) and (3) of the split as the header words them);
      private_synchronised: on D, the context on its private stream and synchronised after the binning; hulk_flush_batch_after(D).
    The next step starts at once.  A flush that does not wait sees two empty spectra and skips them silently."""
    import torch
    inputs_are_a_test("six", "own_half", sketch=False)
    other = other_rank_spectra()
    cycles = delay()[0]
    buf = Buffers()
    if mode == "private_synchronised":
        g, a_stream = sketcher(), None
    else:
        a_stream, handle = caller_stream("stream")
        g = sketcher(stream=handle)
    d_stream = torch.cuda.Stream()
    binning = lambda *a: g.bin_reads_device(*a, reads_per_spectrum=I, first_spectrum=0)
    for b in range(NB):
        if a_stream is None:
            synced(buf, own_half(b), 2 * I, binning)
            g.synchronize()
            coll = d_stream
        else:
            with torch.cuda.stream(a_stream):
                buf.bases[:2 * I * L].copy_(pinned(own_half(b), 2 * I), non_blocking=True)
            binning(*buf.args(2 * I))
            coll = d_stream if mode == "second_stream" else a_stream
            if coll is d_stream:
                d_stream.wait_stream(a_stream)
        with torch.cuda.stream(coll):
            torch.cuda._sleep(cycles)
            spectra_view(g)[2:4].copy_(other[b], non_blocking=True)
        g.flush_batch(T, after_stream=None if mode == "own_stream" else d_stream.cuda_stream)
    g.finish()
    got = results(g)
    g.close()
    # (the context was given half of the reads: its read / minimizer counters are half the oracle's, and the comparators')
    assert_three_yardsticks(got, "six", "after", counters=False)
    assert got["counters"]["n_reads"] == NB * 2 * I


def test_switching_streams_in_mid_run():
    """Case 5.  Two batches on the private stream, hulk_set_stream, two late ones on the caller's, hulk_set_private_stream, two
    more and the ragged tail."""
    inputs_are_a_test("whole", "decoy_even")
    xs, handle = caller_stream("stream")
    buf = Buffers()
    g = sketcher()
    calls = pieces(EVEN)
    for first, n in calls[0:2]:
        synced(buf, first, n, g.add_reads_device)
    g.set_stream(handle)
    for first, n in calls[2:4]:
        late(buf, xs, first, n, g.add_reads_device)
    g.set_private_stream()
    for first, n in calls[4:]:
        synced(buf, first, n, g.add_reads_device)
    g.finish()
    got = results(g)
    g.close()
    assert_three_yardsticks(got, "whole", "even")


@pytest.mark.parametrize("kind", ["stream", "null"])
def test_host_buffers_on_a_callers_stream_context(kind):
    """Case 6.  hulk_add_reads: the staging copies go to the caller's stream and are forked to lane 1 from there."""
    xs, handle = caller_stream(kind)
    g = sketcher(stream=handle)
    for first, n in pieces(EVEN):
        g.add_reads(real()[first * L:(first + n) * L], OFFS[:n + 1])
    g.finish()
    got = results(g)
    g.close()
    assert_oracle(got, oracle("whole"))
    assert_same_bits(got, reference("even", 0), "against the device-buffer context")
