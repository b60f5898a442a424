"""k_minimizer_fast with the wave's reads staged ONCE as 2-bit codes (code stream) and their marks (flag stream): every
alignment of a read in the streams, every kind of mark and where it may stand, two groups per read, the end of a device
buffer, and waves that do not fit the staged span — against the CPU oracle: k-mer spectrum identical, minimizer count equal
(as tests/test_gpu_k1a_set.py, sketch size 1, a few hundred to a few thousand reads per case).

The profiling build's read hook (hulk_debug_read) does not reach the count of deferred reads, so "padding behind the last
read defers nothing" is checked by result only: a deferred read gives the same values through the generic kernel."""
import numpy as np
import pytest

from conftest import pack_reads
from oracle import pyorc

pytestmark = pytest.mark.gpu

IUPAC = b"RYKMSWBDHVN"


def acgt(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])


def put(s, pos, byte):
    b = bytearray(s); b[pos] = byte; return bytes(b)


def compare(seqs, k, w, cuts=None):
    """Spectrum and minimizer count of the GPU against the oracle; cuts: read counts of the separate add_reads calls
    (each call's last read ends its buffer exactly)."""
    import hulk_amd
    o = pyorc.Sketcher(k, w, 1, 0, 1.0, 0)
    g = hulk_amd.GpuSketcher(k, w, 1)
    try:
        bases, offsets = pack_reads(seqs)
        o.add_reads(bases, offsets)
        a = 0
        for c in (cuts or [len(seqs)]):
            b, off = pack_reads(seqs[a:a + c]); a += c
            g.add_reads(b, off)
        assert a == len(seqs)
        oc, gc = o.counters(), g.counters()
        print(f"k={k} w={w} reads={len(seqs)} n_minimizers oracle={oc['n_minimizers']} gpu={gc['n_minimizers']}")
        assert gc["n_reads"] == oc["n_reads"] == len(seqs)
        assert gc["n_minimizers"] == oc["n_minimizers"]
        assert np.array_equal(g.histogram(), o.histogram().astype(np.uint32))
    finally:
        g.close(); o.close()


# ---- every alignment -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,w", [(21, 9), (31, 9), (21, 7), (21, 12), (21, 4)])
def test_every_alignment_of_reads_and_windows(k, w):
    """Uniform lengths 149 .. 165, one call per length: within a wave read i starts at i * L, so the windows fall on every
    bit offset of the code stream.  A wave of such a call starts at a multiple of 16 bases, so every length gets a second
    call whose FIRST read is s = L - 149 bases longer: all later waves' first base then stands at offset s mod 16 of its
    16-byte chunk.  (w = 4: reads of these lengths have more positions than the kernel takes and go to the generic kernel;
    lengths 69 .. 84 are added, which it takes.)"""
    rng = np.random.default_rng(7000 + 100 * k + w)
    seqs, cuts = [], []
    lengths = list(range(149, 166)) + (list(range(69, 85)) if w == 4 else [])
    for L in lengths:
        s = (L - 149) % 17
        seqs += [acgt(rng, L) for _ in range(40)]; cuts.append(40)
        seqs += [acgt(rng, L + s)] + [acgt(rng, L) for _ in range(56)]; cuts.append(57)
    compare(seqs, k, w, cuts)


# ---- marks -----------------------------------------------------------------------------------------------------------------

def marked_reads(rng, L, n_each=24):
    """Reads of L bases with every kind of mark, each among clean neighbours (L is no multiple of 16, so neighbouring reads
    share a 16-byte chunk)."""
    out = []
    def clean(): return acgt(rng, L)
    for _ in range(n_each):
        # N at a read's first / last base: for the read in front the base right behind its end, for the read behind the
        # previous read's last base (its flag stands at position -1 of that read's first block and must read as zero)
        out += [clean(), put(clean(), 0, ord("N")), clean(), put(clean(), L - 1, ord("N")), clean()]
        out += [put(put(clean(), 0, ord("N")), L - 1, ord("N")), put(put(clean(), 0, ord("n")), L - 1, ord("n"))]
        # N anywhere, two N, a run of N
        out += [put(clean(), int(rng.integers(0, L)), ord("N"))]
        s = bytearray(clean()); a = int(rng.integers(0, L - 12)); s[a:a + int(rng.integers(2, 12))] = b"N" * 11; out.append(bytes(s[:L]))
        # lower case, mixed case
        out += [clean().lower(), bytes(c | 0x20 if rng.integers(0, 2) else c for c in clean())]
        # U / u is T
        out += [clean().replace(b"T", b"U"), clean().lower().replace(b"t", b"u")]
        # IUPAC letters (code 4 like N), upper and lower case
        s = bytearray(clean())
        for q in rng.integers(0, L, size=3): s[q] = IUPAC[int(rng.integers(0, len(IUPAC)))] | (0x20 if rng.integers(0, 2) else 0)
        out.append(bytes(s))
        # other bytes that are code 4: punctuation, digits, high bytes
        out += [put(clean(), int(rng.integers(0, L)), int(b)) for b in (ord("-"), ord("*"), ord("7"), 0xFF, 0x80, 0x1F, 0x04)]
        # the raw bytes 0 .. 3 (the reference takes them as codes; this kernel hands the read to the generic one), also at
        # a read's first and last base where the chunk is shared with a clean neighbour
        for b in range(4):
            out += [clean(), put(clean(), int(rng.integers(0, L)), b), clean()]
        out += [clean(), put(clean(), 0, 1), clean(), put(clean(), L - 1, 2), clean()]
        # a raw byte and an N in one read
        out.append(put(put(clean(), 5, 3), 77, ord("N")))
    return out


@pytest.mark.parametrize("k,w,L", [(21, 9, 150), (31, 9, 150), (21, 12, 150), (21, 9, 157), (21, 4, 80), (15, 9, 150)])
def test_marks_of_every_kind(k, w, L):
    """(k, w) = (21, 12): a 16-position block, no N variant — every mark defers; (15, 9): the rolling form's N variant."""
    rng = np.random.default_rng(7100 + 100 * k + w + L)
    seqs = marked_reads(rng, L)
    compare(seqs, k, w)
    order = rng.permutation(len(seqs))
    compare([seqs[i] for i in order], k, w, [1, 15, 16, 17, 33, len(seqs) - 82])


@pytest.mark.parametrize("k", (21, 31))
def test_one_marked_trip_per_wave(k):
    """Waves of 16 reads in which exactly one read — so exactly one of the wave's four trips — carries a mark: an N in
    read r of wave r, a raw byte in read r of wave 16 + r, clean waves between them."""
    rng = np.random.default_rng(7200 + k)
    seqs = []
    for kind in (ord("N"), 2):
        for r in range(16):
            wave = [acgt(rng, 150) for _ in range(16)]
            wave[r] = put(wave[r], int(rng.integers(0, 150)), kind)
            seqs += wave + [acgt(rng, 150) for _ in range(16)]
    compare(seqs, k, 9)


@pytest.mark.parametrize("n", (1, 15, 16, 17, 33))
def test_small_calls_with_marks(n):
    """Calls of 1, 15, 16, 17 and 33 reads, clean and with a mark in the call's last read (at its last base too)."""
    rng = np.random.default_rng(7300 + n)
    seqs, cuts = [], []
    for last in (None, (149, ord("N")), (149, 1), (0, ord("N")), (70, ord("R"))):
        part = [acgt(rng, 150) for _ in range(n)]
        if last: part[-1] = put(part[-1], last[0], last[1])
        seqs += part; cuts.append(n)
    compare(seqs, 21, 9, cuts)


# ---- two groups per read ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (21, 31))
def test_pair_marks_around_the_second_groups_first_block(k):
    """Lengths 260 .. 300 at w = 9: the second group of a pair starts at position 16w - (w-1) = 136; the flag of its base
    p0 - 1 = 135 is the stream's previous position.  An N (and a raw byte) at and around 135, and around the bases where
    the first group's part ends (16w + k - 2) and 16-base borders near them."""
    rng = np.random.default_rng(7400 + k)
    w = 9
    spots = sorted({133, 134, 135, 136, 137, 143, 144, 145, 127, 128, 16 * w - 1, 16 * w, 16 * w + k - 3, 16 * w + k - 2, 16 * w + k - 1, 0, 259})
    seqs = []
    for L in range(260, 301, 4):
        for p in spots:
            seqs += [put(acgt(rng, L), p, ord("N")), acgt(rng, L)]
        seqs += [put(acgt(rng, L), 135, 3), put(put(acgt(rng, L), 135, ord("N")), 136, ord("N")), put(acgt(rng, L), L - 1, ord("N"))]
    compare(seqs, k, w)
    lens = rng.integers(260, 301, size=600)
    mixed = [acgt(rng, int(x)) for x in lens]
    for i in range(0, 600, 7):
        mixed[i] = put(mixed[i], int(rng.integers(120, 160)), ord("N"))
    compare(mixed, k, w, [1, 15, 16, 17, 33, 518])


# ---- end of a device buffer ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", (150, 280))
def test_end_of_a_device_buffer(L):
    """Through add_reads_device: the last read ends the buffer exactly (numel no multiple of 16), or is followed inside the
    buffer by 16 bytes of 0x00, 'N', 0xFF, 0x01 that belong to no read.  The same result in all cases, the oracle's."""
    import torch
    import hulk_amd
    rng = np.random.default_rng(7500 + L)
    k, w, n = 21, 9, 203
    seqs = [acgt(rng, L) for _ in range(n)]
    seqs[-1] = put(seqs[-1], L - 1, ord("N")) if L == 280 else seqs[-1]
    bases, offsets = pack_reads(seqs)
    assert len(bases) % 16 != 0
    o = pyorc.Sketcher(k, w, 1, 0, 1.0, 0)
    o.add_reads(bases, offsets)
    want_n, want_h = o.counters()["n_minimizers"], o.histogram().astype(np.uint32)
    o.close()
    off_d = torch.from_numpy(offsets.astype(np.int64)).cuda()
    for pad in (None, 0x00, ord("N"), 0xFF, 0x01):
        buf = bases if pad is None else np.concatenate([bases, np.full(16, pad, dtype=np.uint8)])
        b_d = torch.from_numpy(buf.copy()).cuda()
        torch.cuda.synchronize()
        g = hulk_amd.GpuSketcher(k, w, 1)
        try:
            g.add_reads_device(b_d.data_ptr(), off_d.data_ptr(), n, L, b_d.numel())
            c = g.counters()
            print(f"L={L} pad={pad} n_minimizers oracle={want_n} gpu={c['n_minimizers']}")
            assert c["n_reads"] == n and c["n_minimizers"] == want_n
            assert np.array_equal(g.histogram(), want_h)
        finally:
            g.close()
        torch.cuda.synchronize()


# ---- waves that do not fit the staged span ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (21, 31))
def test_long_waves_mixed_with_staged_ones(k):
    """Lengths 200 .. 256: 16 such reads exceed the staged span of 3,072 bytes (from 192 bases on average), so those waves
    load per trip from global memory; waves of 150-base reads between them are staged.  With marks in both kinds."""
    rng = np.random.default_rng(7600 + k)
    seqs = []
    for i in range(40):
        long_wave = [acgt(rng, int(rng.integers(200, 257))) for _ in range(16)]
        short_wave = [acgt(rng, 150) for _ in range(16)]
        if i % 3 == 0:
            long_wave[i % 16] = put(long_wave[i % 16], int(rng.integers(0, 200)), ord("N"))
            short_wave[(i + 5) % 16] = put(short_wave[(i + 5) % 16], int(rng.integers(0, 150)), ord("N"))
        if i % 7 == 0:
            long_wave[3] = put(long_wave[3], 199, 1)
        seqs += long_wave + short_wave
    seqs += [acgt(rng, 256) for _ in range(5)]                    # the call ends in a wave of five long reads
    compare(seqs, k, 9)
