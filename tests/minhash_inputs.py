"""The yardstick and the inputs of the MinHash tests (tests/test_minhash_cpu.py, tests/test_gpu_minhash.py, tests/test_gpu_minhash_sizes.py);
no test lives here.

kmv_reference / khf_reference are minhash.KMVsketch / KHFsketch (src/minhash/kmv.go:39-71, khf.go:34-45) restated in numpy, fed with
what the boss's collector feeds the k-mer spectrum: the distinct minimizers of every read, oracle.pyorc.minimizers(read, k, w).

The inputs below are made for the sizes at which the feed changes its code: every step of k_mh_scan's dispatch on S and the size just
above it, the cap of 4096, and the line 2k + 8 + ceil(log2 S) = 64 between the min-reduction and the brute-force KHF feed.  Every
check_* function asserts, on the reference alone, that an input exercises what it claims; a failure says "the inputs are no test"."""
import functools

import numpy as np

from conftest import pack_reads
from oracle import pyorc

U64_MAX = (1 << 64) - 1
NO_TEST = "the inputs are no test: "

W = 9
NUM_BINS = 4096                 # the MinHash sketches do not depend on it, the size of a context's CWS tables (S x bins) does
CAP = 4096                      # HULK_MINHASH_MAX_SKETCH
# the steps of k_mh_scan's dispatch (64 * NS >= S, NS = 1 .. 64), the size above each — the top lanes' slots lie behind S there — and the cap
DISPATCH_SIZES = (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096)
CAP_SIZES = (4095, 4096)
PATHS = ("list", "generic", "table")


# ---- the reference, restated (ONE definition: the test modules import it from here)
def kmv_reference(vals, sketch_size):
    """KMVsketch.AddHash over `vals` + GetSketch: a max-heap of sketch_size entries WITHOUT de-duplication (kmv.go:39-71), so the
    min(sketch_size, len(vals)) smallest values of the multiset, ascending (kmv.go:161-169)."""
    return np.sort(np.asarray(vals, dtype=np.uint64), kind="stable")[:sketch_size]


def khf_reference(vals, sketch_size, chunk=1 << 14):
    """KHFsketch.AddHash over `vals`: slot i = min over x of (x + i * x) mod 2^64, MaxUint64 to begin with (khf.go:20-45)."""
    vals = np.asarray(vals, dtype=np.uint64)
    mult = np.arange(1, sketch_size + 1, dtype=np.uint64)[None, :]
    out = np.full(sketch_size, U64_MAX, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for lo in range(0, len(vals), chunk):
            out = np.minimum(out, (vals[lo:lo + chunk, None] * mult).min(axis=0))
    return out


def khf_merge_reference(a, b):
    return np.minimum(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))      # khf.go:49-55


def khf_naive(vals, sketch_size):
    """(i + 1) * min(x) mod 2^64: what the signature is where no product wraps, and what a feed that takes the min-reduction gives"""
    vals = np.asarray(vals, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return vals.min() * np.arange(1, sketch_size + 1, dtype=np.uint64)


# ---- reads and what they feed
def n_reads(seed, n, lo, hi, n_frac=0.0):
    """n random reads of lo..hi bases; a fraction of them carries N (code 4) and lower-case bases"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(rng.integers(lo, hi + 1)))].copy()
        if rng.random() < n_frac:
            s[rng.integers(0, len(s), size=3)] = ord("N")
            s[rng.integers(0, len(s), size=5)] |= 32
        out.append(s.tobytes())
    return out


def read_values(reads, k, w=W):
    """the AddHash arguments of every read, one array a read"""
    return [pyorc.minimizers(r, k, w) for r in reads]


def fed_values(bases, offsets, k, w=W):
    """every AddHash argument of the stream, in read order"""
    raw = np.ascontiguousarray(bases, dtype=np.uint8).tobytes()
    off = [int(x) for x in offsets]
    parts = read_values([raw[off[i]:off[i + 1]] for i in range(len(off) - 1)], k, w)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)


def frozen(a):
    a.setflags(write=False)
    return a


# ---- A1. the three binning paths, for every size of the dispatch -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def path_reads():
    """list: clean 150-base reads (k_minimizer_fast's list, k_mh_scan<NS, false>); generic: 600 .. 1000 bases, most with N (the
    queue drain of k_minimizer_bin); table: one contig of 20 kb, more than the generic kernel's 1024 positions (the set table of the
    long path, k_mh_scan<NS, true>)"""
    return {"list": n_reads(4101, 400, 150, 150), "generic": n_reads(4102, 30, 600, 1000, n_frac=0.7), "table": n_reads(4103, 1, 20000, 20000)}


@functools.lru_cache(maxsize=None)
def path_inputs(k):
    """{path: (bases, offsets, values)} and, under "all", the values of the three one behind the other"""
    out = {}
    for name, reads in path_reads().items():
        bases, offsets = pack_reads(reads)
        out[name] = (frozen(bases), frozen(offsets), frozen(fed_values(bases, offsets, k)))
    out["all"] = (None, None, frozen(np.concatenate([out[p][2] for p in PATHS])))
    return out


@functools.lru_cache(maxsize=None)
def path_reference(k, name):
    """(KMV, KHF) of a path's values at the cap.  Entry i of either does not depend on the sketch size (the S smallest values are the
    first S of the 4096 smallest; slot i is a minimum over the values alone), so every smaller size is a prefix: sliced()"""
    vals = path_inputs(k)[name][2]
    return frozen(kmv_reference(vals, CAP)), frozen(khf_reference(vals, CAP, chunk=1 << 11))


def sliced(ref, S):
    return ref[0][:S], ref[1][:S]


def check_path_inputs(k):
    c = path_inputs(k)
    reads = path_reads()
    assert all(len(r) == 150 and not set(r) - set(b"ACGT") for r in reads["list"]), NO_TEST + "a list read the fast kernel defers"
    assert all(600 <= len(r) <= 1000 for r in reads["generic"]) and sum(b"N" in r for r in reads["generic"]) >= 10, NO_TEST + "generic reads"
    assert all(len(r) - k + 1 > 1024 for r in reads["table"]), NO_TEST + "the contig fits the generic kernel"
    for name in PATHS:
        assert len(c[name][2]) > 2000, NO_TEST + f"the {name} path feeds {len(c[name][2])} values"
    assert len(c["list"][2]) > 2 * CAP, NO_TEST + "the list path alone does not fill the largest sketch twice over"
    assert len(c["all"][2]) < 25000, "the reference of a test grew: about 16,000 values x 4096 slots was the plan"
    # the prefix rule of path_reference, on the definition itself
    for S in (65, 2049):
        kmv, khf = sliced(path_reference(k, "generic"), S)
        assert np.array_equal(kmv, kmv_reference(c["generic"][2], S)) and np.array_equal(khf, khf_reference(c["generic"][2], S))


def check_wrap_decides(k=31):
    """k = 31: in more than half of the slots of every size the wrap decides, so a feed that took the min-reduction, or lost a lane's
    slots, cannot pass"""
    for name in PATHS + ("all",):
        vals = path_inputs(k)[name][2]
        khf = path_reference(k, name)[1]
        naive = khf_naive(vals, CAP)
        for S in DISPATCH_SIZES:
            differ = int((khf[:S] != naive[:S]).sum())
            assert 2 * differ > S, NO_TEST + f"k {k} {name} S {S}: {differ} slots differ from (i+1) * min(x)"
            top = int((khf[S - (S - 1) % 64 - 1:S] != U64_MAX).sum())
            assert top == (S - 1) % 64 + 1, NO_TEST + "a slot of the last 64-slot block was never set"


def check_no_wrap(k=21):
    """k = 21: 2k + 8 + 12 = 62 <= 64, the shortcut at every size up to the cap, and the reference agrees that it is one"""
    for name in PATHS + ("all",):
        assert np.array_equal(path_reference(k, name)[1], khf_naive(path_inputs(k)[name][2], CAP)), NO_TEST + f"a product wraps at k = {k}"


# ---- A2. KMV at the cap ------------------------------------------------------------------------------------------------------------
CAP_STREAMS = ("fewer", "more", "twice")


@functools.lru_cache(maxsize=None)
def cap_stream(k, name):
    """[(bases, offsets)] to add one after the other, and the values they feed: fewer values than S, more values than S, and the same
    reads twice, so that every value occurs twice"""
    reads = path_reads()["list"]
    if name == "fewer":
        calls = [pack_reads(reads[:100])]
    elif name == "more":
        calls = [pack_reads(reads)]
    else:
        calls = [pack_reads(reads), pack_reads(reads)]
    vals = np.concatenate([fed_values(b, o, k) for b, o in calls])
    return calls, frozen(vals)


def check_cap_streams(k):
    for S in CAP_SIZES:
        fewer, more, twice = (cap_stream(k, n)[1] for n in CAP_STREAMS)
        assert 1000 < len(fewer) < S - 64, NO_TEST + f"'fewer' feeds {len(fewer)} values"
        assert len(more) > S + 64 and len(twice) == 2 * len(more), NO_TEST + f"'more' feeds {len(more)} values"
        srt = np.sort(twice)
        assert (srt[0:2 * S:2] == srt[1:2 * S:2]).all() and (srt[1:2 * S - 1:2] < srt[2:2 * S:2]).all(), NO_TEST + "the low values do not come in pairs"
    # S = 4095 is odd: the bound lies between the two copies of one value — entry S - 1 is the (S + 1)-th smallest fed value too, and
    # the strict '<' of the feed (the second copy is no smaller than the bound) decides that the slot keeps one copy
    S = 4095
    ref = kmv_reference(twice, S)
    assert ref[S - 1] == np.sort(twice)[S] and ref[S - 2] < ref[S - 1], NO_TEST + "the bound does not fall between two copies"
    assert kmv_reference(twice, 4096)[4095] == ref[S - 1], NO_TEST + "at 4096 the pair is whole"


# ---- A3. the order of the reads ----------------------------------------------------------------------------------------------------
ORDERS = ("descending", "ascending", "shuffled")
ORDER_SIZES = (1025, 4096)


@functools.lru_cache(maxsize=None)
def ordered_reads(k, order):
    """the list path's reads by their smallest minimizer: descending — every read brings a value below everything fed before it, which
    enters at rank 0 and carries an entry through every 64-entry block of the KMV array —, ascending, and shuffled"""
    reads = path_reads()["list"]
    lows = np.array([int(v.min()) for v in read_values(reads, k)], dtype=np.uint64)
    asc = np.argsort(lows, kind="stable")
    idx = {"ascending": asc, "descending": asc[::-1], "shuffled": np.random.default_rng(4104).permutation(len(reads))}[order]
    return [reads[i] for i in idx]


def bound_falls(per_read, S):
    """in how many reads the running bound kmv[S - 1] (MaxUint64 while fewer than S values are held) ends below where it began"""
    held, bound, falls = np.zeros(0, dtype=np.uint64), U64_MAX, 0
    for v in per_read:
        held = np.sort(np.concatenate([held, v]))[:S]
        now = int(held[S - 1]) if len(held) == S else U64_MAX
        falls += now < bound
        bound = now
    return falls


def check_orders(k):
    ref = sorted(path_reads()["list"])
    for order in ORDERS:
        assert sorted(ordered_reads(k, order)) == ref
    desc = read_values(ordered_reads(k, "descending"), k)
    lows = [int(v.min()) for v in desc]
    assert all(a >= b for a, b in zip(lows, lows[1:])) and len(set(lows)) > len(lows) - 8, NO_TEST + "the reads' smallest values do not descend"
    for S in ORDER_SIZES:
        falls = bound_falls(desc, S)
        assert 2 * falls >= len(desc), NO_TEST + f"S {S}: the bound falls in {falls} of {len(desc)} reads"
    return desc


# ---- A4. the line between the two KHF feeds ----------------------------------------------------------------------------------------
# hulk_create takes the min-reduction when 2k + 8 + ceil(log2 S) <= 64: S_lo = 2^(64 - 2k - 8) is the largest such size.  w = 1: every
# k-mer is its own window, the fed values fill the whole range below 2^(2k + 8), and products wrap as soon as the rule allows them to
# (with w = 9 a minimizer is the smallest of nine hashes and the line is all but invisible).
BOUNDARY_W = 1
BOUNDARY_S_LO = {23: 1024, 24: 256, 25: 64, 26: 16, 27: 4, 28: 1}
# default_rng seeds of 300 reads of 150 bases, the first per k for which all three conditions of check_boundary hold (searched on the
# reference by find_boundary_seed)
BOUNDARY_SEEDS = {23: 5, 24: 5, 25: 9, 26: 6, 27: 5, 28: 5}


def boundary_sizes(k):
    """S_lo (the last size of the min-reduction), S_lo + 1 (the first of the brute force: its last slot alone can wrap), 2 * S_lo - 1
    (the largest size whose log2 a floor and a ceiling tell apart) and 2 * S_lo (a quarter of the upper half wraps)"""
    lo = BOUNDARY_S_LO[k]
    return sorted({lo, lo + 1, max(lo, 2 * lo - 1), 2 * lo})


@functools.lru_cache(maxsize=None)
def boundary_input(k, seed=None):
    reads = n_reads(BOUNDARY_SEEDS[k] if seed is None else seed, 300, 150, 150)
    bases, offsets = pack_reads(reads)
    vals = fed_values(bases, offsets, k, BOUNDARY_W)
    return frozen(bases), frozen(offsets), frozen(vals)


def boundary_conditions(k, seed=None):
    """(holds at S_lo, wrapped slots above S_lo at 2 * S_lo, the last slot of S_lo + 1 differs), on the reference"""
    lo = BOUNDARY_S_LO[k]
    assert 64 - 2 * k - 8 == lo.bit_length() - 1
    vals = boundary_input(k, seed)[2]
    khf, naive = khf_reference(vals, 2 * lo), khf_naive(vals, 2 * lo)
    return bool((khf[:lo] == naive[:lo]).all()), int((khf[lo:] != naive[lo:]).sum()), bool(khf[lo] != naive[lo])


def find_boundary_seed(k, first=5, tries=200):
    for seed in range(first, first + tries):
        holds, wrapped, last = boundary_conditions(k, seed)
        if holds and 4 * wrapped >= BOUNDARY_S_LO[k] and last:
            return seed
    raise AssertionError(NO_TEST + f"no seed in {tries} for k = {k}")


def check_boundary(k):
    lo = BOUNDARY_S_LO[k]
    vals = boundary_input(k)[2]
    assert int(vals.max()) < 1 << (2 * k + 8) and int(vals.max()) >= 1 << (2 * k + 7), NO_TEST + "the values do not fill the range below 2^(2k + 8)"
    holds, wrapped, last = boundary_conditions(k)
    assert holds, NO_TEST + f"k {k}: a product wraps at S_lo = {lo}, where the rule says none can"
    assert 4 * wrapped >= lo, NO_TEST + f"k {k}: {wrapped} of the {lo} slots above S_lo differ from (i+1) * min(x) at 2 * S_lo"
    assert last, NO_TEST + f"k {k}: the last slot of S_lo + 1 = {lo + 1} is (i+1) * min(x): a feed on the wrong side of the line passes"
    assert find_boundary_seed(k) == BOUNDARY_SEEDS[k], "BOUNDARY_SEEDS is not what the search finds"
    return wrapped
