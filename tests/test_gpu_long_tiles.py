"""k_long_tile when a workgroup owns several tiles of a sequence.

launch_long_group (hulk_minimizer.hip) gives every sequence of a group at most max(1, 262144 / n_seqs) workgroups, at most 65535:
a sequence with more tiles than that is covered by workgroups that loop over tiles, reusing their LDS state (the staged codes, the
hashes, the queue q and its length qn) from one tile to the next.  Assemblies (thousands of contigs) and chromosomes land there.
Every case below asserts through a mirror of the host's launch rules that it really reaches a second trip of that loop, and compares
with the CPU oracle, or (140 Mbp) with the profiling build's two-pass kernels, which flush once per workgroup."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import pack_reads
from oracle import pyorc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hulk_amd", "csrc")
EXP_LIB = os.path.join(CSRC, "libhulkhip_exp.so")

# ---- the launch geometry of the long-sequence path, as the host computes it
# hulk_api.hip: hulk_add_reads stages host chunks of <= 2^19 reads / 96 MiB; hulk_add_reads_device hands at most
#   batch * interval reads (interval > 0) and at most MAX_READS_PER_LAUNCH (hulk_ctx.h) to one bin_reads
# hulk_flush.hip bin_long_reads: sequences of more than GENERIC_XCAP_MAX k-mer positions, in groups of <= GROUP_POS positions
#   and <= GROUP_SEQS sequences
# hulk_minimizer.hip launch_long_group: bx = min(ceil(max_npos / TP), max(1, 262144 / n_seqs), 65535), TP = LONG_TILE - roundup8(w)
CHUNK_READS, CHUNK_BYTES = 1 << 19, 96 << 20
MAX_READS_PER_LAUNCH = 4 << 20
GENERIC_XCAP_MAX, GROUP_POS, GROUP_SEQS = 1024, 128 << 20, 32768
LONG_TILE, GRID_WORKGROUPS, GRID_X = 2048, 262144, 65535


def tile_span(w):
    """TP: the positions a tile reports (the first roundup8(w) of its LONG_TILE are context)"""
    return LONG_TILE - (max(w, 1) + 7) // 8 * 8


def bin_calls(lens, interval=0, batch=16):
    """the read ranges [a, b) of the bin_reads calls that ONE hulk_add_reads of these lengths makes on a fresh context"""
    cum = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])
    calls, i0, n, seq_count = [], 0, len(lens), 0
    while i0 < n:
        i1 = i0
        while i1 < n and i1 - i0 < CHUNK_READS and (i1 == i0 or cum[i1 + 1] - cum[i0] <= CHUNK_BYTES):
            i1 += 1
        pos = i0
        while pos < i1:
            chunk = i1 - pos
            if interval:
                chunk = min(chunk, batch * interval - seq_count % interval)
            chunk = min(chunk, MAX_READS_PER_LAUNCH)
            calls.append((pos, pos + chunk))
            seq_count += chunk
            pos += chunk
        i0 = i1
    return calls


def long_groups(lens, k, calls):
    """the groups of read indices that bin_long_reads launches, in order"""
    groups = []
    for a, b in calls:
        cur, pos_total = [], 0
        for i in range(a, b):
            if lens[i] < k or lens[i] - k + 1 <= GENERIC_XCAP_MAX:
                continue
            npos = lens[i] - k + 1
            if cur and (pos_total + npos > GROUP_POS or len(cur) >= GROUP_SEQS):
                groups.append(cur)
                cur, pos_total = [], 0
            cur.append(i)
            pos_total += npos
        if cur:
            groups.append(cur)
    return groups


def tile_trips(lens, k, w, calls):
    """{read index: (workgroups per sequence bx, trips of its workgroups over its tiles)} for the reads of the long path"""
    TP, out = tile_span(w), {}
    for g in long_groups(lens, k, calls):
        max_npos = max(lens[i] - k + 1 for i in g)
        bx = min(-(-max_npos // TP), max(1, GRID_WORKGROUPS // len(g)), GRID_X)
        for i in g:
            tiles = -(-(lens[i] - k + 1) // TP)
            out[i] = (bx, -(-tiles // bx))
    return out


def test_the_mirror_follows_the_sources():
    """the constants of the mirror above are the ones the library is built with"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("hulk_api.hip", "hulk_flush.hip", "hulk_minimizer.hip", "hulk_ctx.h")}
    assert "CHUNK_READS = 1ull << 19, CHUNK_BYTES = 96ull << 20;" in src["hulk_api.hip"]
    assert "if (I) { const uint64_t room = (uint64_t)c->T * I - fill; if (chunk > room) chunk = room; }" in src["hulk_api.hip"]
    assert "MAX_READS_PER_LAUNCH = 4u << 20;" in src["hulk_ctx.h"]
    assert "GENERIC_XCAP_MAX = 1024;" in src["hulk_flush.hip"]
    assert "GROUP_POS = 128ull << 20;" in src["hulk_flush.hip"] and "GROUP_SEQS = 32768;" in src["hulk_flush.hip"]
    assert "(pos_total + npos > GROUP_POS || descs.size() >= GROUP_SEQS)" in src["hulk_flush.hip"]
    m = src["hulk_minimizer.hip"]
    assert "constexpr int LONG_TILE = 2048;" in m
    body = m[m.index("// tiles per sequence: enough for the longest"):m.index('prof_mark(s, "k_long_tile")')]
    assert "(((uint64_t)(P.w ? P.w : 1) + 7) & ~7ull), TP = (uint64_t)LONG_TILE - H;" in body
    assert re.search(r"bx = \(max_npos \+ TP - 1\) / TP;\s+const uint64_t cap = std::max<uint64_t>\(1, 262144 / n_seqs\);"
                     r"\s+if \(bx > cap\) bx = cap;\s+if \(bx > 65535\) bx = 65535;", body)


# ---- inputs
def grouped_input(seed, k, w, n_short, short_lens, long_lens, long_at, tail=300, interval=0, batch=16):
    """n_short sequences just past the one-wave kernel (short_lens: length range) with long ones at the fractions long_at of the
    list, and `tail` short reads behind them.  The bases around the tile borders that the second trip of a workgroup covers get N
    (code 4) and lower case.  Returns (bases, offsets, {long read index: (bx, trips)})."""
    rng = np.random.default_rng(seed)
    lens = list(rng.integers(short_lens[0], short_lens[1] + 1, size=n_short))
    for f, L in sorted(zip(long_at, long_lens), reverse=True):
        lens.insert(int(round(f * n_short)), L)
    lo = w + k - 1
    lens += list(rng.integers(lo, max(lo, 400) + 1, size=tail))
    lens = [int(x) for x in lens]
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(offsets[-1]))]
    trips = tile_trips(lens, k, w, bin_calls(lens, interval, batch))
    TP, H = tile_span(w), (max(w, 1) + 7) // 8 * 8
    longs = {i: trips[i] for i in trips if lens[i] >= min(long_lens)}
    assert len(longs) == len(long_lens)
    for i, (bx, n_trips) in longs.items():
        assert n_trips >= 2, f"read {i} ({lens[i]} bases): {n_trips} trip(s) of bx = {bx} workgroups"
        s = bases[int(offsets[i]):int(offsets[i + 1])]             # (a view)
        for t in range(bx, min(bx + 3, -(-(lens[i] - k + 1) // TP))):
            border = t * TP                                        # first position tile t reports; its context starts H before
            lower = slice(max(0, border - H - 5), min(len(s), border + 11))
            s[lower] += 32
            for at in (border - H, border - 1, border, border + k - 1, border + k):
                if 0 <= at < len(s) and rng.random() < 0.6:
                    s[at] = ord("N")
    return bases, offsets, longs


def assert_same_run(o, g, interval):
    """spectrum, counters, then (after finish) the sketch and the count-min counters"""
    gh, oh = g.histogram(), o.histogram()
    assert np.array_equal(gh, oh.astype(np.uint32)), f"{int((gh != oh).sum())} bins differ"
    n_min = o.counters()["n_minimizers"]
    assert g.counters()["n_minimizers"] == n_min
    if interval == 0:
        assert int(gh.sum(dtype=np.uint64)) == n_min, "spectrum increments lost"
    o.finish(); g.finish()
    om, ow = o.sketch()
    gm, gw = g.sketch()
    assert np.array_equal(gm, om), f"{int((gm != om).sum())} of {len(om)} mins differ"
    assert np.allclose(gw, ow, rtol=1e-9, atol=0)
    assert np.array_equal(g.cms(), o.cms()), "count-min counters differ"
    oc, gc = o.counters(), g.counters()
    for key in ("n_reads", "n_minimizers", "total_len"):
        assert oc[key] == gc[key], key


# (k, w) with context H = 8 (w 1, 9), 16 and 256; n_short sequences of a group of one call cap the grid, the long ones take two
# trips.  The oracle's per-read set is a linear scan (quadratic in a sequence's distinct minimizers): long ones stay <= 250 kb.
CASES = {
    "k21_w9": dict(k=21, w=9, n_short=8000, short_lens=(1100, 1500), long_lens=(80_000, 80_000), long_at=(0.3, 0.8)),
    "k15_w255": dict(k=15, w=255, n_short=3000, short_lens=(1100, 1500), long_lens=(250_000, 250_000), long_at=(0.0, 0.5)),
    "k11_w1": dict(k=11, w=1, n_short=8000, short_lens=(1040, 1100), long_lens=(70_000,), long_at=(0.6,)),
    "k31_w16": dict(k=31, w=16, n_short=8000, short_lens=(1100, 1500), long_lens=(80_000, 80_000), long_at=(0.2, 1.0),
                    num_bins=300007),
    # one group of 8000 sequences over 8 spectra of the ring (the long ones in spectra 1 and 6), one work lane
    "k21_w9_interval": dict(k=21, w=9, n_short=7998, short_lens=(1100, 1500), long_lens=(80_000, 80_000), long_at=(0.19, 0.81),
                            interval=1000, batch=8, work_lanes=1),
    # two groups, one per batch, on the two work lanes (one table and descriptor scratch: the lanes' groups are ordered)
    "k15_w255_two_lanes": dict(k=15, w=255, n_short=15996, short_lens=(1040, 1200), long_lens=(70_000,) * 4,
                               long_at=(0.1, 0.4, 0.6, 0.9), interval=1000, batch=8, work_lanes=2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_grouped_long_sequences_loop_over_tiles(name):
    """Shipping build, default grid: a group of thousands of 1.0-1.5 kb sequences caps the workgroups per sequence (bx 32 or 87),
    so the long sequences of the group are covered by workgroups that run two or more tiles — the regime of assemblies.  One call
    per input; spectrum bit-exact, minimizer count, spectrum sum = count (interval 0), sketch and count-min counters."""
    import hulk_amd
    c = dict(CASES[name])
    k, w = c.pop("k"), c.pop("w")
    num_bins, interval, batch, lanes = c.pop("num_bins", 0), c.pop("interval", 0), c.pop("batch", 16), c.pop("work_lanes", 0)
    bases, offsets, longs = grouped_input(100 * k + w, k, w, interval=interval, batch=batch, **c)
    S = 16
    g = hulk_amd.GpuSketcher(k, w, S, interval, 1.0, num_bins, batch=batch if interval else 0, work_lanes=lanes)
    g.add_reads(bases, offsets)
    o = pyorc.Sketcher(k, w, S, num_bins, 1.0, interval)
    o.add_reads(bases, offsets)
    assert_same_run(o, g, interval)
    g.close(); o.close()


# ---- the profiling build: grid capped by HULK_LONG_TILE_GRID, waves 1-3 late to the flush with HULK_LONG_TILE_LAG
_EXP_RUNNER = """
import json, os, sys, hashlib
import numpy as np
sys.path.insert(0, {root!r})
import torch, hulk_amd
from hulk_amd import _lib
assert _lib.load().hulk_build_info().endswith(b" experiments=1")
d = np.load(sys.argv[1])
for env in json.loads(sys.argv[2]):
    for key in ("HULK_LONG_TILE_GRID", "HULK_LONG_TILE_LAG"):
        os.environ.pop(key, None)
    os.environ.update(env)
    g = hulk_amd.GpuSketcher({k}, {w}, 4, num_bins={num_bins})
    g.add_reads(d["bases"], d["offsets"])
    h = g.histogram()
    print(json.dumps([hashlib.md5(h.tobytes()).hexdigest(), int(h.sum(dtype=np.uint64)), g.counters()["n_minimizers"]]), flush=True)
    g.close()
"""


def test_profiling_build_strided_tiles_with_late_waves(tmp_path):
    """A handful of 20-150 kb sequences and short reads through the profiling build with at most 1 or 3 workgroups per sequence
    (HULK_LONG_TILE_GRID): one workgroup strides over up to 74 tiles.  HULK_LONG_TILE_LAG holds waves 1-3 back ~40 us between the
    barrier in front of a tile's flush and their read of the queue length — a reset of qn that is not ordered behind those reads
    then loses their share of every tile but the last.  Spectrum and minimizer count against the oracle (computed here)."""
    if not os.path.exists(EXP_LIB):
        pytest.skip("profiling build (libhulkhip_exp.so) not built")
    k, w, num_bins = 21, 9, 0
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
    p = np.array([0.24] * 4 + [0.009] * 4 + [0.004])
    seqs = [bytes(acgt[rng.choice(len(acgt), size=L, p=p)]) for L in (20_000, 47_000, 96_000, 150_000)]
    seqs += [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(L))]) for L in rng.integers(29, 900, size=60)]
    order = rng.permutation(len(seqs))
    bases, offsets = pack_reads([seqs[i] for i in order])
    np.savez(str(tmp_path / "in.npz"), bases=bases, offsets=offsets)
    o = pyorc.Sketcher(k, w, 4, num_bins, 1.0, 0)
    o.add_reads(bases, offsets)
    oh = o.histogram().astype(np.uint32)
    want = [hashlib.md5(oh.tobytes()).hexdigest(), o.counters()["n_minimizers"], o.counters()["n_minimizers"]]
    o.close()
    configs = [{"HULK_LONG_TILE_GRID": "1", "HULK_LONG_TILE_LAG": "1"}, {"HULK_LONG_TILE_GRID": "3", "HULK_LONG_TILE_LAG": "1"},
               {"HULK_LONG_TILE_GRID": "2"}]
    code = _EXP_RUNNER.format(root=ROOT, k=k, w=w, num_bins=num_bins)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.npz"), json.dumps(configs)],
                       env=dict(os.environ, HULK_LIB="exp"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [json.loads(line) for line in r.stdout.split("\n") if line.startswith("[")]
    assert len(got) == len(configs)
    for env, res in zip(configs, got):
        assert res == want, f"{env}: (md5, spectrum sum, n_minimizers) {res} != the oracle's {want}"


_TWO_PASS_RUNNER = """
import sys, hashlib
sys.path.insert(0, {root!r})
import numpy as np, torch, hulk_amd
from hulk_amd import _lib, synth
assert _lib.load().hulk_build_info().endswith(b" experiments=1")
b, off = synth.reads_torch({first}, 1, {L})
torch.cuda.synchronize()
g = hulk_amd.GpuSketcher(21, 9, 8)
g.add_reads_device(b.data_ptr(), off.data_ptr(), 1, {L}, b.numel())
h = g.histogram()
print("RESULT", hashlib.md5(h.tobytes()).hexdigest(), int(h.sum(dtype=np.uint64)), g.counters()["n_minimizers"], flush=True)
g.close()
"""


def test_chromosome_scale_sequence():
    """One synthetic 140 Mbp sequence through hulk_add_reads_device: bx = 65535 workgroups for 68,898 tiles, so the first
    3,363 workgroups run two.  Spectrum sum = minimizer count, and spectrum and count equal those of the profiling build's
    two-pass kernels (HULK_LONG_TWO_PASS: one flush per workgroup; pinned to the oracle by
    test_gpu_parity.py::test_long_tile_kernel_at_its_tile_borders).  Too large for the CPU oracle."""
    import torch
    import hulk_amd
    from hulk_amd import synth
    first, L = 31, 140_000_000
    trips = tile_trips([L], 21, 9, bin_calls([L]))
    assert trips[0] == (65535, 2)
    b, off = synth.reads_torch(first, 1, L)
    torch.cuda.synchronize()
    g = hulk_amd.GpuSketcher(21, 9, 8)
    g.add_reads_device(b.data_ptr(), off.data_ptr(), 1, L, b.numel())
    g.synchronize()
    del b, off
    h = g.histogram()
    n_min = g.counters()["n_minimizers"]
    g.close()
    assert n_min > L // 10
    assert int(h.sum(dtype=np.uint64)) == n_min, "spectrum increments lost"
    if not os.path.exists(EXP_LIB):
        pytest.skip("profiling build (libhulkhip_exp.so) not built: no two-pass comparator")
    code = _TWO_PASS_RUNNER.format(root=ROOT, first=first, L=L)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HULK_LIB="exp", HULK_LONG_TWO_PASS="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    md5, hsum, nmin = [l for l in r.stdout.split("\n") if l.startswith("RESULT ")][-1].split()[1:]
    assert (md5, int(hsum), int(nmin)) == (hashlib.md5(h.tobytes()).hexdigest(), n_min, n_min)


def test_assembly_fasta_through_the_device_parser(tmp_path):
    """An assembly-shaped FASTA file (9,000 contigs of 1.1-1.6 kb and five of 80 kb, 60-80 columns per line) through
    sketch_files(fasta=True) on the default device parser, which hands a file this size to the sketcher as ONE batch: one group
    of 9,005 sequences, bx = 29, the 80 kb contigs take two trips.  Sketch, spectrum and counters against the oracle over the
    reference's line pump."""
    import hulk_amd
    from oracle import linepump
    k, w, S = 21, 9, 16
    rng = np.random.default_rng(5)
    lens = [int(x) for x in rng.integers(1100, 1601, size=9000)]
    for at in (8500, 6000, 4500, 2000, 10):
        lens.insert(at, 80_000)
    trips = tile_trips(lens, k, w, [(0, len(lens))])
    assert {trips[i] for i in trips if lens[i] == 80_000} == {(29, 2)}
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    p = str(tmp_path / "assembly.fa")
    with open(p, "wb") as fh:
        for i, L in enumerate(lens):
            s = acgt[rng.integers(0, 4, size=L)].tobytes()
            width = int(rng.integers(60, 81))
            fh.write(b">contig_%d len=%d\n" % (i, L) + b"\n".join(s[j:j + width] for j in range(0, L, width)) + b"\n")
    g = hulk_amd.GpuSketcher(k, w, S)
    st = g.sketch_files([p], fasta=True)
    seqs = linepump.sequences([p], fasta=True)
    assert st["n_seqs"] == len(seqs) == len(lens) and [len(s) for s in seqs] == lens
    o = pyorc.Sketcher(k, w, S)
    o.add_reads(*pack_reads(seqs))
    assert_same_run(o, g, 0)
    g.close(); o.close()
