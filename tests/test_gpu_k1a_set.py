"""k_minimizer_fast's per-read set as a table of 32-bit candidate indices: the branches of the set phase and the staging's
end-of-buffer rules, on the instances built for five workgroups per CU (k = 21 and k = 31 at w = 9), one group per read
(150 bases) and two (280 bases), against the CPU oracle: k-mer spectrum identical, minimizer count equal.

The set phase has three outcomes per candidate: slot empty (new), slot holding a candidate of EQUAL value (a duplicate:
the compare-load finds it), slot holding another value (probe on).  Random reads give the first and the third (27 values
in 128 slots collide in most reads); the second needs the same k-mer at two run starts of one read, which the inputs
below are built to contain — and are checked to contain, on the oracle alone, before the GPU sees them."""
import numpy as np
import pytest

from conftest import pack_reads
from oracle import pyorc

pytestmark = pytest.mark.gpu

W = 9
KS = (21, 31)
LENGTHS = (150, 280)          # one 16-lane group per read / two (PAIR)
N_UNITS = 200                 # two-halves reads drawn per (k, length)
# (k, L) -> how many of the N_UNITS reads U + U (|U| = L / 2, seeds below) satisfy n(U + U) < 2 n(U) on the oracle, each read
# sketched alone: the condition that the read really holds a duplicate minimizer.  Nearly all do, except at k = 31 with
# 75-base halves, where the junction adds about as many new minimizers as the repeat removes.  The reads that do not are
# left out BEFORE anything runs on the GPU (counts recorded here from the oracle on the CPU); every kept read is compared.
KEPT = {(21, 150): 199, (21, 280): 200, (31, 150): 150, (31, 280): 200}


def acgt(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])


def n_min(seq, k):
    return len(pyorc.minimizers(seq, k, W))


def two_halves(k, L):
    """N_UNITS reads U + U with |U| = L / 2 (fixed seed), and those of them that really hold a duplicate minimizer:
    n(U + U) < 2 n(U), each read sketched alone on the oracle."""
    rng = np.random.default_rng(9000 + 10 * k + L)
    units = [acgt(rng, L // 2) for _ in range(N_UNITS)]
    kept = [u + u for u in units if n_min(u + u, k) < 2 * n_min(u, k)]
    return units, kept


def spacer_repeats(rng, k, L, n):
    """A unit of k + 12 bases, a spacer, the unit again, ... up to L bases: the unit's minimizers return at later run starts."""
    out = []
    for _ in range(n):
        unit, s = acgt(rng, k + 12), b""
        while len(s) < L:
            s += unit + acgt(rng, int(rng.integers(3, 20)))
        out.append(s[:L])
    return out


def compare(seqs, k, cuts=None):
    """Spectrum and minimizer count of the GPU against the oracle; cuts: read counts of the separate add_reads calls."""
    import hulk_amd
    o = pyorc.Sketcher(k, W, 4, 0, 1.0, 0)
    g = hulk_amd.GpuSketcher(k, W, 4)
    try:
        bases, offsets = pack_reads(seqs)
        o.add_reads(bases, offsets)
        if cuts is None:
            g.add_reads(bases, offsets)
        else:
            assert sum(cuts) == len(seqs)
            a = 0
            for c in cuts:
                part = seqs[a:a + c]; a += c
                b, off = pack_reads(part)               # its last read ends the buffer exactly
                g.add_reads(b, off)
        oc, gc = o.counters(), g.counters()
        print(f"k={k} reads={len(seqs)} n_minimizers oracle={oc['n_minimizers']} gpu={gc['n_minimizers']}")
        assert gc["n_reads"] == oc["n_reads"] == len(seqs)
        assert gc["n_minimizers"] == oc["n_minimizers"]
        assert np.array_equal(g.histogram(), o.histogram().astype(np.uint32))
    finally:
        g.close(); o.close()


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k", KS)
def test_two_identical_halves(k, L):
    """Occupied by an equal value: reads U + U.  The condition on the inputs is asserted on the oracle alone."""
    units, kept = two_halves(k, L)
    print(f"k={k} L={L}: generated {len(units)}, kept {len(kept)}")
    assert len(units) == N_UNITS and len(kept) == KEPT[(k, L)]
    for s in kept:
        assert n_min(s, k) < 2 * n_min(s[:L // 2], k)
    compare(kept, k)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k", KS)
def test_unit_repeated_with_spacers(k, L):
    rng = np.random.default_rng(9100 + 10 * k + L)
    seqs = spacer_repeats(rng, k, L, 600)
    # the inputs do contain duplicates: fewer distinct minimizers per read than a random read of the length has
    dup = sum(n_min(s, k) for s in seqs[:100])
    rnd = sum(n_min(acgt(rng, L), k) for _ in range(100))
    assert dup < rnd
    compare(seqs, k)


@pytest.mark.parametrize("k", KS)
def test_halves_shared_across_the_two_groups_of_a_pair(k):
    """280 bases: the second group of a pair starts at position 136.  V + U + V + U' with |V + U| = 140 puts the same
    k-mers in both groups' parts (each finds the other's candidates in the shared table)."""
    rng = np.random.default_rng(9200 + k)
    seqs = []
    for _ in range(500):
        u = acgt(rng, 140)
        seqs.append(u + u)                                        # the halves coincide with the groups' parts (nearly)
        a, b = acgt(rng, 90), acgt(rng, 50)
        seqs.append(a + b + a + acgt(rng, 50))                    # the first group's start returns in the second's part
        seqs.append(acgt(rng, 50) + a + acgt(rng, 50) + a)        # ... and the other way round
    assert all(len(s) == 280 for s in seqs)
    assert sum(n_min(s, k) for s in seqs[:60]) < sum(n_min(acgt(rng, 280), k) for _ in range(60))
    compare(seqs, k)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k", KS)
def test_random_batches_collide_in_the_table(k, L):
    """Occupied by another value, probe on: a few thousand random reads."""
    rng = np.random.default_rng(9300 + 10 * k + L)
    compare([acgt(rng, L) for _ in range(4000)], k)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k", KS)
def test_one_n_and_low_complexity_around_the_deferral_limit(k, L):
    """A read with one N stays in the kernel; low-complexity reads (short periods with a few substitutions, two- and
    three-letter alphabets, homopolymers) are the ones with the most equal values per read and the ones that come nearest
    to the limit of 64 run starts per group, above which a read is deferred whole to the generic kernel.  (At w = 9 a
    group's 144 positions start a run about every fifth position whatever the sequence; the deferral itself, unchanged
    here, is exercised at w = 2 by test_repetitive_reads_fall_back_to_generic_kernel.)"""
    rng = np.random.default_rng(9400 + 10 * k + L)
    seqs = []
    for i in range(300):
        s = bytearray(acgt(rng, L)); s[int(rng.integers(0, L))] = ord("N"); seqs.append(bytes(s))
    for period in (1, 2, 3, 5, 7, 11, 13, 17, 23, 29, 37, 41, 47, 53, 61, 67, 71):
        for _ in range(12):
            unit = acgt(rng, period)
            s = bytearray((unit * (L // period + 1))[:L])
            for q in rng.integers(0, L, size=int(rng.integers(0, 4))):     # a few substitutions: run starts come and go
                s[q] = b"ACGT"[int(rng.integers(0, 4))]
            seqs.append(bytes(s))
    for alphabet in (b"AC", b"AT", b"ACG"):                                 # few letters: many equal k-mers per read
        a = np.frombuffer(alphabet, dtype=np.uint8)
        seqs += [bytes(a[rng.integers(0, len(a), size=L)]) for _ in range(60)]
    seqs += [b"A" * L, b"AC" * (L // 2), b"ACG" * (L // 3) + b"A" * (L % 3)]
    seqs += [acgt(rng, L) for _ in range(200)]
    order = rng.permutation(len(seqs))
    compare([seqs[i] for i in order], k)


@pytest.mark.parametrize("k", KS)
def test_read_counts_off_sixteen_and_mixed_lengths(k):
    """The staging's end-of-buffer rules: calls of 1, 15, 17, 31, 1000 + 7 reads, each call's last read ending its buffer
    exactly; and reads of every length from 30 (k = 31: from the shortest legal read, w + k - 1 = 39) to 256 in one wave, so
    that some waves' reads do not fit the staged span and take the loads from global memory."""
    rng = np.random.default_rng(9500 + k)
    cuts = [1, 15, 17, 31, 1007, 3, 16, 33]
    seqs = [acgt(rng, 150) for _ in range(sum(cuts))]
    compare(seqs, k, cuts)
    lo = max(30, k + W - 1)
    mixed = [acgt(rng, int(rng.integers(lo, 257))) for _ in range(3001)]
    compare(mixed, k, [2000, 1001])
    longer = [acgt(rng, int(rng.integers(200, 257))) for _ in range(1003)]     # 16 reads of > 196 bases exceed the staged span
    compare(longer, k, [1003])
